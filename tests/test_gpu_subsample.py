"""Subsampling on the device (-m gpu): the *_sub kernels of vgmi_fastq.hip / vgmi_fasta.hip / vgmi_bam.hip and everything above them.

The oracle is the rule itself: counting file G with (F, S) must equal counting G' with the option off, G' = G with exactly the dropped
reads removed (subsample_cases.py).  Counters, node counters, histogram, records, bases and masked bases are compared with those of G';
n_seen must be the file's reads, consumed the file's length and stopped False -- every record has been taken by the DEVICE, so the
host reader's form of the rule cannot make these tests green.  Then the hand-overs, where device and host share a file and one
numbering, the refusals, and the CLI against the unmodified reference run on the filtered files."""
import gzip
import os

import ctypes as C
import numpy as np
import pytest

import bam_cases as BC
import bam_py as B
import quality_mask_cases as Q
import subsample_cases as S
from conftest import GOLDEN, get_cohort
from varigraph_amd import host, synth, vgmi

pytestmark = pytest.mark.gpu

_TEXT = b"@HD\tVN:1.6\tSO:unsorted\n"
N_FASTQ, N_FASTA, N_BAM = 600, 300, 300
CASES = [(f, s) for f in S.FRACTIONS for s in S.SEEDS]
IDS = [f"F{f}-S{s}" for f, s in CASES]


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


_haps, _fastq, _want = {}, {}, {}


def _hap(cohort):
    name = cohort.meta["name"]
    if name not in _haps:
        _haps[name] = cohort.haplotypes()
    return _haps[name]


def _fastq_case(cohort, seed):
    """the FASTQ case of `seed`: 600 records, two of 20 000 bases where F = 0.5 keeps one and drops the other"""
    key = (cohort.meta["name"], seed)
    if key not in _fastq:
        _fastq[key] = S.fastq_records(_hap(cohort), N_FASTQ, seed, S.long_positions(seed, N_FASTQ))
    return _fastq[key]


def _run(ctx, call):
    ctx.counts_reset()
    r = call()
    cov, node, hist = ctx.counts_finish(nodes=True, hist=True)
    return r, (cov, node, hist)


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


def _bgzf(tmp_path, name, data, block=0xff00):
    src, dst = tmp_path / (name + ".txt"), tmp_path / (name + ".gz")
    src.write_bytes(data)
    synth.bgzf_compress_file(str(src), str(dst), level=4, block=block)
    return dst.read_bytes()


def _check(got, want, n_file, n_kept, file_len, what, n_bases=None):
    """got: G with the option; want: G' without"""
    print(f"{what}: kept {got['n_records']} of {got.get('n_seen')} (model {n_kept} of {n_file}), bases {got['n_bases']}, consumed {got['consumed']}")
    assert not got["stopped"] and not want["stopped"], what
    assert got["n_seen"] == n_file and got["n_kept"] == n_kept, what
    assert (got["n_records"], got["n_bases"]) == (want["n_records"], want["n_bases"]), what
    assert got["n_records"] == n_kept and (n_bases is None or got["n_bases"] == n_bases), what
    assert got["consumed"] == file_len, what
    assert got["masked_bases"] == want["masked_bases"], what
    assert "n_seen" not in want


# ---- FASTQ -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f,seed", CASES, ids=IDS)
def test_fastq_text_equals_counting_the_filtered_file(f, seed, gc, monkeypatch):
    """plain text, whole and in 4 KiB chunks: at 0.02 most chunks keep nothing, the 20 000-base records are carried across five chunks,
    one kept and one dropped (at 0.5)"""
    g, ctx, cohort = gc
    recs = _fastq_case(cohort, seed)
    kept = S.kept_of(recs, f, seed)
    G, GP = S.fastq_text(recs), S.fastq_text(kept)
    for chunk_kb in (None, 4):
        m = _chunked(monkeypatch, chunk_kb)
        try:
            got, c_got = _run(ctx, lambda: ctx.fastq_text(G, subsample=(f, seed)))
            want, c_want = _run(ctx, lambda: ctx.fastq_text(GP))
            plain, c_plain = _run(ctx, lambda: ctx.fastq_text(G))
        finally:
            m.__exit__(None, None, None)
        _check(got, want, len(recs), len(kept), len(G), (f, seed, chunk_kb), sum(len(r[1]) for r in kept))
        assert got["tail"] == b"" and plain["n_records"] == len(recs)
        _same_counts(c_got, c_want, (f, seed, chunk_kb))
        assert not np.array_equal(c_plain[0], c_got[0])         # the case shows something: the whole file counts differently


@pytest.mark.parametrize("f,seed", CASES, ids=IDS)
def test_fastq_chunk_ends_behind_a_kept_and_behind_a_dropped_record(f, seed, gc):
    """commits that end right behind a dropped record and right behind a kept one (the next chunk then starts with the other kind as
    often as not), and a file without its final newline: the last record is the host reader's"""
    g, ctx, cohort = gc
    recs = _fastq_case(cohort, seed)[:140]
    mask = S.kept_mask(len(recs), f, seed)
    kept = S.kept_of(recs, f, seed)
    G, GP = S.fastq_text(recs), S.fastq_text(kept)
    cuts = {"behind_kept": next(i for i in range(20, 140) if mask[i]), "behind_dropped": next(i for i in range(20, 140) if not mask[i]),
            "first_dropped": next(i for i in range(20, 139) if not mask[i + 1]), "first_kept": next(i for i in range(20, 139) if mask[i + 1])}
    want, c_want = _run(ctx, lambda: ctx.fastq_text(GP))
    for name, i in cuts.items():
        cut = S.end_of_record(recs, i)
        got, c_got = _run(ctx, lambda: ctx.fastq_text(G, piece=cut, subsample=(f, seed)))
        _check(got, want, len(recs), len(kept), len(G), (f, seed, name))
        _same_counts(c_got, c_want, (f, seed, name))
    got, c_got = _run(ctx, lambda: ctx.fastq_text(G[:-1], subsample=(f, seed)))
    want, c_want = _run(ctx, lambda: ctx.fastq_text(S.fastq_text(S.kept_of(recs[:-1], f, seed) + recs[-1:])[:-1]))
    assert not got["stopped"] and got["n_seen"] == len(recs) - 1 and got["tail"] == want["tail"] == S.fastq_text(recs[-1:])[:-1]
    assert (got["n_records"], got["n_bases"]) == (want["n_records"], want["n_bases"]) and got["n_records"] == int(mask[:-1].sum())
    _same_counts(c_got, c_want, (f, seed, "no final newline"))


def test_fraction_one_through_the_setter_is_the_stream_that_never_called_it(gc, monkeypatch):
    g, ctx, cohort = gc
    recs = _fastq_case(cohort, 11)
    G = S.fastq_text(recs)
    for chunk_kb in (None, 4):
        m = _chunked(monkeypatch, chunk_kb)
        try:
            plain, c_plain = _run(ctx, lambda: ctx.fastq_text(G))
            one, c_one = _run(ctx, lambda: ctx.fastq_text(G, subsample=(1.0, 11)))
            back, c_back = _run(ctx, lambda: ctx.fastq_text(G, subsample=[(0.5, 11), (1.0, 7)]))      # the last value set holds
            half, c_half = _run(ctx, lambda: ctx.fastq_text(G, subsample=[(1.0, 11), (0.5, 11)]))
        finally:
            m.__exit__(None, None, None)
        for r, c in ((one, c_one), (back, c_back)):
            assert (r.pop("n_seen"), r.pop("n_kept")) == (len(recs), len(recs))
            assert r == plain
            _same_counts(c, c_plain, "F = 1")
        assert half["n_records"] == int(S.kept_mask(len(recs), 0.5, 11).sum()) < len(recs) and half["n_seen"] == len(recs)
        assert not np.array_equal(c_half[0], c_plain[0])


@pytest.mark.parametrize("f", S.FRACTIONS)
def test_block_gzip_and_gzip_equal_counting_the_filtered_file(f, gc, tmp_path, monkeypatch):
    g, ctx, cohort = gc
    monkeypatch.delenv("VGMI_FASTQ_CHUNK_KB", raising=False)
    seed = 11
    recs = _fastq_case(cohort, seed)
    kept = S.kept_of(recs, f, seed)
    G, GP = S.fastq_text(recs), S.fastq_text(kept)
    want, c_want = _run(ctx, lambda: ctx.fastq_text(GP))
    comp = _bgzf(tmp_path, "g", G, block=3000)          # members of 3 000 bytes of text: records lie across members
    got, c_got = _run(ctx, lambda: ctx.fastq_bgzf(comp, subsample=(f, seed)))
    assert not got["inflate_failed"] and got["taken"] == len(comp) and got["tail"] == b""
    _check(got, want, len(recs), len(kept), len(G), (f, "bgzf"))
    _same_counts(c_got, c_want, (f, "bgzf"))
    got, c_got = _run(ctx, lambda: ctx.fastq_gzip(gzip.compress(G, 6), subsample=(f, seed)))
    assert (got["stop"], got["reason"], got["device_text_bytes"]) == (1, 0, len(G))
    _check(got, want, len(recs), len(kept), len(G), (f, "gzip"))
    _same_counts(c_got, c_want, (f, "gzip"))


@pytest.mark.parametrize("first", (False, True), ids=["quality_then_subsample", "subsample_then_quality"])
def test_with_a_minimum_base_quality_in_either_setter_order(first, gc, monkeypatch):
    """F = 0.5 with min_quality = 20: the kept reads masked, the dropped ones not looked at -- FASTQ in 4 KiB chunks, and BAM"""
    g, ctx, cohort = gc
    f, seed = 0.5, 11
    recs = _fastq_case(cohort, seed)
    kept = S.kept_of(recs, f, seed)
    masked, total = Q.masked_records(kept, 20)
    assert 0 < total < Q.masked_records(recs, 20)[1]
    G, GP = S.fastq_text(recs), S.fastq_text(masked)
    for chunk_kb in (None, 4):
        m = _chunked(monkeypatch, chunk_kb)
        try:
            got, c_got = _run(ctx, lambda: ctx.fastq_text(G, min_quality=20, subsample=(f, seed), subsample_first=first))
            want, c_want = _run(ctx, lambda: ctx.fastq_text(GP))
        finally:
            m.__exit__(None, None, None)
        assert got["masked_bases"] == total
        got["masked_bases"] = 0
        _check(got, want, len(recs), len(kept), len(G), (first, chunk_kb))
        _same_counts(c_got, c_want, (first, chunk_kb))
    brecs = S.bam_records(_hap(cohort), N_BAM, seed)
    gp, n_reads = S.bam_filtered(brecs, f, seed)
    bmasked, btotal = Q.masked_bam_records(gp, 20)
    raw, hlen, _ = B.raw_bam(brecs, text=_TEXT)
    comp, comp_p = B.bgzf_stored(raw, [])[0], B.bgzf_stored(B.raw_bam(bmasked, text=_TEXT)[0], [])[0]
    got, c_got = _run(ctx, lambda: ctx.bam_bgzf(comp, hlen, 0, min_quality=20, subsample=(f, seed), subsample_first=first))
    want, c_want = _run(ctx, lambda: ctx.bam_bgzf(comp_p, hlen, 0))
    assert got["masked_bases"] == btotal > 0
    got["masked_bases"] = 0
    _check(got, want, n_reads, B.reads_block(gp)[1], len(raw), (first, "bam"))
    _same_counts(c_got, c_want, (first, "bam"))


# ---- FASTA -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f,seed", CASES, ids=IDS)
def test_fasta_single_line_and_wrapped(f, seed, gc, monkeypatch):
    """the device never takes a FASTA stream's last record (only the end of the data completes it): it is the tail on both sides, and the
    records in front of it are numbered 0 .. n - 2"""
    g, ctx, cohort = gc
    recs = S.fastq_records(_hap(cohort), N_FASTA, seed + 100)
    kept = S.kept_of(recs[:-1], f, seed)
    for width in (None, 60):
        G, GP = S.fasta_text(recs, width), S.fasta_text(kept + recs[-1:], width)
        last = S.fasta_text(recs[-1:], width)
        for chunk_kb in (None, 4):
            m = _chunked(monkeypatch, chunk_kb)
            try:
                got, c_got = _run(ctx, lambda: ctx.fasta_text(G, subsample=(f, seed)))
                want, c_want = _run(ctx, lambda: ctx.fasta_text(GP))
                plain, c_plain = _run(ctx, lambda: ctx.fasta_text(G))
            finally:
                m.__exit__(None, None, None)
            _check(got, want, len(recs) - 1, len(kept), len(G) - len(last), (f, seed, width, chunk_kb), sum(len(r[1]) for r in kept))
            assert got["tail"] == want["tail"] == last
            _same_counts(c_got, c_want, (f, seed, width, chunk_kb))
            assert not np.array_equal(c_plain[0], c_got[0])


# ---- BAM ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f,seed", CASES, ids=IDS)
def test_bam_numbers_the_reads_not_the_records(f, seed, gc, tmp_path, monkeypatch):
    """secondary, supplementary and SEQ '*' records between the reads; whole, and with members of 3 000 bytes in 4 KiB chunks"""
    g, ctx, cohort = gc
    recs = S.bam_records(_hap(cohort), N_BAM, seed)
    gp, n_reads = S.bam_filtered(recs, f, seed)
    raw, _, _ = B.raw_bam(recs, text=_TEXT)
    _, n_kept, n_bases = B.reads_block(gp)
    for chunk_kb, block in ((None, 0xff00), (4, 3000)):
        hlen, _ = B.write_bam(tmp_path / "g.bam", recs, text=_TEXT, block=block)
        B.write_bam(tmp_path / "gp.bam", gp, text=_TEXT, block=block)
        comp, comp_p = (tmp_path / "g.bam").read_bytes(), (tmp_path / "gp.bam").read_bytes()
        m = _chunked(monkeypatch, chunk_kb)
        try:
            got, c_got = _run(ctx, lambda: ctx.bam_bgzf(comp, hlen, 0, subsample=(f, seed)))
            want, c_want = _run(ctx, lambda: ctx.bam_bgzf(comp_p, hlen, 0))
            plain, c_plain = _run(ctx, lambda: ctx.bam_bgzf(comp, hlen, 0))
        finally:
            m.__exit__(None, None, None)
        assert not got["inflate_failed"] and got["tail"] == b""
        _check(got, want, n_reads, n_kept, len(raw), (f, seed, chunk_kb), n_bases)
        _same_counts(c_got, c_want, (f, seed, chunk_kb))
        assert not np.array_equal(c_plain[0], c_got[0]) and plain["n_records"] == n_reads == N_BAM


@pytest.mark.parametrize("which", ("kept", "dropped"))
def test_bam_split_at_every_chunk_end_alignment(which, gc):
    """One small stream with the non-reads interleaved, cut into two chunks at every alignment of a read -- one the rule keeps, one it
    drops -- against the chunk's end that bam_cases.py enumerates (SWEEP): the first chunk ends inside the record in front, at its
    boundary, inside its block_size, its fixed fields, its name.  The read's rank in the file must come through the carry."""
    g, ctx, cohort = gc
    f, seed = 0.5, 11
    recs = S.bam_records(_hap(cohort), 40, seed)
    numbers, i = {}, 0
    for j, r in enumerate(recs):
        if r.kept:
            numbers[j] = i
            i += 1
    at = next(j for j in range(12, len(recs)) if j in numbers and S.keep(numbers[j], seed, f) == (which == "kept") and len(recs[j].seq) > 60)
    gp, n_reads = S.bam_filtered(recs, f, seed)
    _, n_kept, n_bases = B.reads_block(gp)
    whole = BC.Case("subsample_whole", "subsample", gp, refs=())
    want, c_want = _run(ctx, lambda: ctx.bam_bgzf(whole.comp, whole.hlen, whole.n_ref, piece=whole.piece))
    offs = BC.Case("subsample_offsets", "subsample", recs, refs=()).offs
    for d in BC.SWEEP:
        case = BC.Case("subsample_sweep", "subsample", recs, refs=(), cuts=[offs[at] - d])
        got, c_got = _run(ctx, lambda: ctx.bam_bgzf(case.comp, case.hlen, case.n_ref, piece=case.piece, subsample=(f, seed)))
        _check(got, want, n_reads, n_kept, len(case.raw), (which, d), n_bases)
        _same_counts(c_got, c_want, (which, d))


# ---- the hand-overs: device and host reader share a file and one numbering ---------------------------------------------------------------
def _sample(g, ctx, paths, monkeypatch, sub=None, q=0, env=None):
    with monkeypatch.context() as m:
        for k in ("VGH_HOST_PARSE", "VGH_HOST_INFLATE", "VGH_DEVICE_GUNZIP", "VGMI_FASTQ_CHUNK_KB"):
            m.delenv(k, raising=False)
        for k, v in (env or {}).items():
            m.setenv(k, v)
        cov, node, hist, st = g.sample_count(ctx, [str(p) for p in paths], threads=4, require_depth=False, min_base_quality=q, subsample=sub)
    return (cov, node, hist), (st["n_reads"], st["read_base"]), (st.get("reads_seen"), st.get("reads_kept")), st["masked_bases"]


@pytest.mark.parametrize("f,seed", [(0.5, 11), (0.5, 7), (0.02, 11)], ids=["F0.5-S11", "F0.5-S7", "F0.02-S11"])
def test_hand_overs_keep_one_numbering(f, seed, gc, tmp_path, monkeypatch):
    """A CRLF record in the middle of the file and no final newline: with 4 KiB chunks the device takes the chunks in front of the CRLF
    record and the host reader goes on at the device's n_seen.  The same file whole through VGH_HOST_PARSE=1, the host's inflate paths,
    and as a pair with a second file of equal record count: the same numbers survive in both."""
    g, ctx, cohort = gc
    recs = list(_fastq_case(cohort, seed))
    mid = len(recs) // 2
    recs[mid] = recs[mid] + ("crlf",)
    kept = S.kept_of(recs, f, seed)
    G, GP = S.fastq_text(recs, final_newline=False), S.fastq_text(kept)
    paths = {}
    for name, data in (("g", G), ("gp", GP)):
        (tmp_path / (name + ".fq")).write_bytes(data)
        (tmp_path / (name + ".fq.gz")).write_bytes(gzip.compress(data, 6))
        (tmp_path / (name + ".bgz.gz")).write_bytes(_bgzf(tmp_path, name + "_b", data))
        paths[name] = {k: tmp_path / (name + ext) for k, ext in (("plain", ".fq"), ("gzip", ".fq.gz"), ("bgzf", ".bgz.gz"))}
    want_c, want_n, none, _ = _sample(g, ctx, [paths["gp"]["plain"]], monkeypatch)
    assert want_n == (len(kept), sum(len(r[1]) for r in kept)) and none == (None, None)
    runs = [("plain", {}), ("plain", {"VGMI_FASTQ_CHUNK_KB": "4"}), ("gzip", {}), ("bgzf", {}), ("plain", {"VGH_HOST_PARSE": "1"}),
            ("bgzf", {"VGH_HOST_PARSE": "1"}), ("bgzf", {"VGH_HOST_INFLATE": "1"}), ("gzip", {"VGH_DEVICE_GUNZIP": "0"})]
    for kind, env in runs:
        c, n, sk, _ = _sample(g, ctx, [paths["g"][kind]], monkeypatch, (f, seed), env=env)
        print(f"F={f} S={seed} {kind} {env}: kept {sk[1]} of {sk[0]} (model {len(kept)} of {len(recs)})")
        assert n == want_n and sk == (len(recs), len(kept)), (kind, env)
        _same_counts(c, want_c, (f, seed, kind, env))
    # the device's share of the chunked run and the host reader's rest add up to the file
    ctx.counts_reset()
    with monkeypatch.context() as m:
        m.setenv("VGMI_FASTQ_CHUNK_KB", "4")
        r = ctx.fastq_text(G, subsample=(f, seed))
    ctx.counts_finish()
    assert r["stopped"] and 0 < r["n_seen"] <= mid and r["n_records"] == int(S.kept_mask(r["n_seen"], f, seed).sum())
    assert r["consumed"] == len(S.fastq_text(recs[:r["n_seen"]]))
    rest = tmp_path / "rest.fq"
    rest.write_bytes(G[r["consumed"]:])
    _, n_host, _, _, nxt = host.reads_read_all_s(str(rest), f, seed, first_number=r["n_seen"])
    assert nxt == len(recs) and r["n_records"] + n_host == len(kept)
    # a pair: two files of equal record count under one seed keep the same numbers
    recs2 = S.fastq_records(_hap(cohort), len(recs), seed + 50)
    (tmp_path / "g2.fq").write_bytes(S.fastq_text(recs2))
    (tmp_path / "gp2.fq").write_bytes(S.fastq_text(S.kept_of(recs2, f, seed)))
    want_c, want_n, _, _ = _sample(g, ctx, [paths["gp"]["plain"], tmp_path / "gp2.fq"], monkeypatch)
    c, n, sk, _ = _sample(g, ctx, [paths["g"]["plain"], tmp_path / "g2.fq"], monkeypatch, (f, seed))
    assert n == want_n and sk == (2 * len(recs), 2 * len(kept))
    _same_counts(c, want_c, (f, seed, "pair"))


def test_bam_and_fasta_hand_overs(gc, tmp_path, monkeypatch):
    """a BAM and a FASTA file through vgh_sample_count_s: the device with the host reader for what it leaves (FASTA: the last record),
    and the host reader alone (VGH_HOST_PARSE=1, VGH_HOST_INFLATE=1)"""
    g, ctx, cohort = gc
    f, seed = 0.5, 7
    recs = S.bam_records(_hap(cohort), N_BAM, seed)
    gp, n_reads = S.bam_filtered(recs, f, seed)
    B.write_bam(tmp_path / "g.bam", recs, text=_TEXT)
    B.write_bam(tmp_path / "gp.bam", gp, text=_TEXT)
    want_c, want_n, _, _ = _sample(g, ctx, [tmp_path / "gp.bam"], monkeypatch)
    for env in ({}, {"VGH_HOST_PARSE": "1"}, {"VGH_HOST_INFLATE": "1"}, {"VGMI_FASTQ_CHUNK_KB": "4"}):
        c, n, sk, _ = _sample(g, ctx, [tmp_path / "g.bam"], monkeypatch, (f, seed), env=env)
        assert n == want_n and sk == (n_reads, want_n[0]), env
        _same_counts(c, want_c, env)
    frecs = S.fastq_records(_hap(cohort), N_FASTA, seed + 100)
    fkept = S.kept_of(frecs, f, seed)
    for width in (None, 60):
        (tmp_path / "g.fa").write_bytes(S.fasta_text(frecs, width))
        (tmp_path / "gp.fa").write_bytes(S.fasta_text(fkept, width))
        want_c, want_n, _, _ = _sample(g, ctx, [tmp_path / "gp.fa"], monkeypatch)
        for env in ({}, {"VGH_HOST_PARSE": "1"}, {"VGMI_FASTQ_CHUNK_KB": "4"}):
            c, n, sk, _ = _sample(g, ctx, [tmp_path / "g.fa"], monkeypatch, (f, seed), env=env)
            assert n == want_n == (len(fkept), sum(len(r[1]) for r in fkept)) and sk == (len(frecs), len(fkept)), (width, env)
            _same_counts(c, want_c, (width, env))


# ---- the refusals ------------------------------------------------------------------------------------------------------------------------
def test_setter_refusals_leave_the_stream_serving(gc):
    g, ctx, cohort = gc
    l = ctx._l
    f, seed = 0.5, 7
    recs = _fastq_case(cohort, seed)
    kept = S.kept_of(recs, f, seed)
    G = S.fastq_text(recs)
    _, c_want = _run(ctx, lambda: ctx.fastq_text(S.fastq_text(kept)))
    for bad in (0.0, -1.0, 1.5, float("nan"), float("inf")):
        with pytest.raises(vgmi.VgmiError) as e:
            ctx.fastq_text(G, subsample=(bad, seed))
        assert e.value.code == vgmi.E_INVALID and "0 < fraction <= 1" in str(e.value)
    ctx.counts_reset()
    fq = C.c_void_p()
    assert l.vgmi_fastq_open(ctx._h, C.byref(fq)) == 0
    for bad in (0.0, 2.0, float("nan")):
        assert l.vgmi_fastq_set_subsample(fq, bad, seed) == vgmi.E_INVALID
        assert b"0 < fraction <= 1" in l.vgmi_last_error(ctx._h)
    assert l.vgmi_fastq_set_subsample(fq, f, seed) == 0          # a valid call after the refusals
    half = len(S.fastq_text(recs[:len(recs) // 2]))
    seen, n_kept = C.c_uint64(), C.c_uint64()
    for lo, hi in ((0, half), (half, len(G))):
        buf, cap = C.c_void_p(), C.c_size_t()
        assert l.vgmi_fastq_acquire(fq, C.byref(buf), C.byref(cap)) == 0
        C.memmove(buf, G[lo:hi], hi - lo)
        assert l.vgmi_fastq_commit(fq, hi - lo) == 0
        assert l.vgmi_fastq_set_subsample(fq, 0.9, seed) == vgmi.E_STATE         # bytes have been committed
        assert l.vgmi_fastq_set_subsample(fq, 1.0, seed) == vgmi.E_STATE
        assert l.vgmi_fastq_subsample_stats(fq, C.byref(seen), C.byref(n_kept)) == 0       # ... and the stream serves on
    assert (seen.value, n_kept.value) == (len(recs), len(kept))
    nr, nb, cons, st = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_int()
    assert l.vgmi_fastq_close(fq, C.byref(nr), C.byref(nb), C.byref(cons), C.byref(st), None, 0, None) == 0
    assert (nr.value, nb.value, cons.value, st.value) == (len(kept), sum(len(r[1]) for r in kept), len(G), 0)
    _same_counts(ctx.counts_finish(nodes=True, hist=True), c_want, "the rule set before the refused calls holds")
    # FASTA and BAM streams take the setter; a stream without it reports its records as seen and kept
    for opener in (lambda q: l.vgmi_fastq_open_fasta(ctx._h, C.byref(q)), lambda q: l.vgmi_fastq_open_bam(ctx._h, 100, 0, C.byref(q)),
                   lambda q: l.vgmi_fastq_open(ctx._h, C.byref(q))):
        fq = C.c_void_p()
        assert opener(fq) == 0
        assert l.vgmi_fastq_set_subsample(fq, 0.25, 3) == 0 and l.vgmi_fastq_set_subsample(fq, -0.25, 3) == vgmi.E_INVALID
        assert l.vgmi_fastq_set_min_quality(fq, 20) == 0 and l.vgmi_fastq_set_subsample(fq, 1.0, 3) == 0
        assert l.vgmi_fastq_subsample_stats(fq, C.byref(seen), C.byref(n_kept)) == 0 and (seen.value, n_kept.value) == (0, 0)
        assert l.vgmi_fastq_close(fq, None, None, None, None, None, 0, None) == 0
    for bad in (0.0, 1.5, float("nan")):
        with pytest.raises(vgmi.VgmiError, match="0 < fraction <= 1"):
            g.sample_count(ctx, [os.path.join(cohort.dir, "reads_1.fq.gz")], subsample=(bad, 11))
    got = g.sample_count(ctx, [os.path.join(cohort.dir, "reads_1.fq.gz")], require_depth=False)
    assert got[3]["n_reads"] == cohort.n_reads // 2
    got = g.sample_count(ctx, [os.path.join(cohort.dir, "reads_1.fq.gz")], require_depth=False, subsample=(1.0, 11))
    assert got[3]["n_reads"] == got[3]["reads_seen"] == got[3]["reads_kept"] == cohort.n_reads // 2


# ---- the CLI against the unmodified reference ------------------------------------------------------------------------------------------
# The VCF lines of the reference on the filtered files, taken on the CPU beforehand: a run that loses or gains a record shows here
# before the byte comparison does.
REF_LINES = {"half": 109, "seed7_use_depth": 109, "quality": 109, "three": [109, 109, 109]}


def _cli_files(work, f, seed, draw=False):
    """cohort_snp's gzip pair (G: the committed files themselves, or -- draw -- with qualities drawn afresh) and the filtered plain files
    the reference reads; -> (G paths, G' paths, [(kept, seen)] per file)"""
    d = os.path.join(GOLDEN, "cohort_snp")
    G, GP, stats = [], [], []
    for mate in (1, 2):
        path = os.path.join(d, f"reads_{mate}.fq.gz")
        text = gzip.open(path, "rb").read()
        if draw:
            text = Q.draw_qualities(text, 200 + mate)
            path = os.path.join(work, f"g_{mate}.fq.gz")
            open(path, "wb").write(gzip.compress(text, 6))
        gp, kept, seen = S.filtered_fastq_text(text, f, seed)
        if draw:
            gp = Q.masked_text(gp, 20)[0]
        G.append(path)
        GP.append(os.path.join(work, f"gp_{mate}_{seed}.fq"))
        open(GP[-1], "wb").write(gp)
        stats.append((kept, seen))
    return G, GP, stats


CLI_CASES = {
    "half": (11, [], [], {}, False),
    "half_host_parse": (11, [], [], {"VGH_HOST_PARSE": "1"}, False),
    "seed7_use_depth": (7, ["--subsample-seed", "7", "--use-depth"], ["--use-depth"], {}, False),
    "quality": (11, ["--min-base-quality", "20"], [], {}, True),
}


@pytest.mark.parametrize("case", list(CLI_CASES))
def test_cli_subsample_equals_the_reference_on_the_filtered_files(case, tmp_path):
    import test_gpu_configs as cfg
    cfg._need_binaries()
    seed, extra, ref_extra, env, draw = CLI_CASES[case]
    d = os.path.join(GOLDEN, "cohort_snp")
    work = str(tmp_path)
    graph = os.path.join(work, "graph.bin")
    open(graph, "wb").write(gzip.open(os.path.join(d, "graph.bin.gz"), "rb").read())
    G, GP, stats = _cli_files(work, 0.5, seed, draw)
    cfg._reference_genotype(os.path.join(work, "ref"), graph, "sample0 " + " ".join(GP) + "\n", ref_extra, threads=4, timeout=25)
    want = cfg._vcf(os.path.join(work, "ref"), "sample0")
    lines = REF_LINES[case.replace("_host_parse", "")]
    print(f"{case}: reference VCF on the filtered files has {want.count(bytes([10]))} lines")
    assert lines is None or want.count(b"\n") == lines
    _, log = cfg._native_genotype(os.path.join(work, "sub"), graph, "sample0 " + " ".join(G) + "\n",
                                  ["--gpu", "0", "--buffer", "8", "--subsample", "0.5"] + extra, threads=4, env=dict(env, VGH_TIMING="1"))
    assert cfg._vcf(os.path.join(work, "sub"), "sample0") == want
    got = sorted((ln.split("': ")[0].split("'")[1], ln.split("': ")[1]) for ln in log.splitlines() if "reads kept (--subsample" in ln)
    assert got == sorted((p, f"{k} of {n} reads kept (--subsample 0.5, seed {seed})") for p, (k, n) in zip(G, stats)), log[-2000:]
    if "VGH_HOST_PARSE" not in env:
        assert log.count("reads from the device-side reader") == 2
    # the unsampled run's VCF is another one
    which = "expected_use_depth.vcf" if "--use-depth" in extra else None
    if which:
        from test_gpu_integration import _strip_gq
        assert _strip_gq(want) != _strip_gq(open(os.path.join(d, which), "rb").read())
    else:
        cfg._native_genotype(os.path.join(work, "off"), graph, "sample0 " + " ".join(G) + "\n", ["--gpu", "0", "--buffer", "8"] + extra, threads=4)
        assert cfg._vcf(os.path.join(work, "off"), "sample0") != want


def test_cli_three_samples_in_one_run(tmp_path):
    """three samples of one run -- the pair, and each mate alone under another name -- each equal to the reference on its filtered files"""
    import test_gpu_configs as cfg
    cfg._need_binaries()
    d = os.path.join(GOLDEN, "cohort_snp")
    work = str(tmp_path)
    graph = os.path.join(work, "graph.bin")
    open(graph, "wb").write(gzip.open(os.path.join(d, "graph.bin.gz"), "rb").read())
    G, GP, _ = _cli_files(work, 0.5, 11)
    cfg_text = lambda p: f"sample0 {p[0]} {p[1]}\nsample1 {p[0]}\nsample2 {p[1]}\n"
    cfg._reference_genotype(os.path.join(work, "ref"), graph, cfg_text(GP), ["--use-depth"], threads=4, timeout=25)
    cfg._native_genotype(os.path.join(work, "sub"), graph, cfg_text(G), ["--gpu", "0", "--buffer", "8", "--subsample", "0.5", "--use-depth"], threads=4)
    n_lines = []
    for s in ("sample0", "sample1", "sample2"):
        want = cfg._vcf(os.path.join(work, "ref"), s)
        n_lines.append(want.count(b"\n"))
        assert cfg._vcf(os.path.join(work, "sub"), s) == want, s
    print("three samples: reference VCF lines", n_lines)
    assert REF_LINES["three"] is None or n_lines == REF_LINES["three"]
