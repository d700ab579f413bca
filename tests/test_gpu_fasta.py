"""FASTA read files on the device (vgmi_fastq_open_fasta, csrc/vgmi_fasta.hip): single-line and wrapped records against the host
reader -- the literal restatement of kseq_read (include/kseq.h:192-232) that test_host_cpu.py pins --, the oracle on the block that
reader returns, and for the CLI the reference binary itself, which reads FASTA through the same kseq."""
import gzip
import os
import shutil

import numpy as np
import pytest

import oracle_lib as o
from conftest import get_cohort
from varigraph_amd import host, synth, vgmi

pytestmark = pytest.mark.gpu


def _reads(n, seed, lo=30, hi=400, hap=None):
    rng = np.random.default_rng(seed)
    if hap is None:
        hap = get_cohort("cohort_snp").haplotypes()[1]
    out = []
    for _ in range(n):
        ln = int(rng.integers(lo, hi))
        s = int(rng.integers(0, len(hap) - ln))
        r = bytearray(hap[s:s + ln].tobytes())
        if rng.random() < 0.1:
            r[int(rng.integers(0, ln))] = ord("N")
        if rng.random() < 0.05:
            r = bytearray(bytes(r).lower())
        out.append(bytes(r))
    return out


def _long_read(n_bytes):
    hap = get_cohort("cohort_snp").haplotypes()[0]
    return np.concatenate([hap] * (n_bytes // hap.size + 1)).tobytes()[:n_bytes]


def _record(i, read, width=None, name=None, rng=None, gaps=False):
    """one FASTA record: width None = single line, an int = wrapped there, "ragged" = line widths drawn from rng; gaps: empty lines
    between its sequence lines and behind it"""
    head = name if name is not None else b">read%d some comment" % i
    lines, p = [], 0
    while p < len(read):
        w = len(read) if width is None else int(rng.integers(1, 120)) if width == "ragged" else width
        lines.append(read[p:p + w])
        p += w
    sep = b"\n\n" if gaps else b"\n"
    return head + b"\n" + sep.join(lines) + (b"\n\n\n" if gaps else b"\n")


def _fasta(reads, width=None, names=None, seed=0, gaps=False):
    rng = np.random.default_rng(seed)
    return b"".join(_record(i, r, width, names[i] if names else None, rng, gaps) for i, r in enumerate(reads))


def _fastq(reads):
    return b"".join(b"@q%d\n%s\n+\n%s\n" % (i, r, b"I" * len(r)) for i, r in enumerate(reads))


def _cases():
    rd = _reads(300, 1)
    odd_names = [[b">a>b", b">@at", b">plus+ +", b">tab\there\tand there", b">", b">> >", b">+"][i % 7] + b"%d" % i for i in range(len(rd))]
    mixed = [(b"@" if i % 3 == 0 else b">") + b"r%d" % i for i in range(len(rd))]
    mixed[0] = b">r0"
    c = {
        "single_line": _fasta(rd),
        "wrapped_60": _fasta(rd, 60),
        "wrapped_70": _fasta(rd, 70),
        "wrapped_80": _fasta(rd, 80),
        "ragged": _fasta(rd, "ragged", seed=2),
        "empty_lines": _fasta(rd, 50, gaps=True),
        "odd_headers": _fasta(rd, 60, names=odd_names),
        "at_headed_records": _fasta(rd, 60, names=mixed),
        "lower_and_n": _fasta([r.lower() if i % 2 else r.replace(b"A", b"N") for i, r in enumerate(rd)], 60),
        "no_trailing_newline": _fasta(rd, 60)[:-1],
        "one_record": _fasta(rd[:1], 60),
        "one_record_single_line_no_newline": _fasta(rd[:1])[:-1],
        "record_200kb_wrapped_80": _fasta(rd[:100], 80) + _record(1000, _long_read(200_000), 80) + _fasta(rd[100:], 80),
        "record_3mib": _fasta(rd[:100], 80) + _record(1000, _long_read(3 << 20), 80) + _fasta(rd[100:], 80),
        "long_single_lines": _fasta([_long_read(20_000 + 37 * i) for i in range(12)]),
        "plus_line_in_record_120": _fasta(rd[:120], 60) + b">bad\n" + rd[120][:60] + b"\n+" + rd[120][60:] + b"\n" + _fasta(rd[121:], 60),
        "empty_record_in_the_middle": _fasta(rd[:150], 60) + b">empty\n\n>next\nACGTACGTACGTACGTACGTACGTACGTACGTACGT\n" + _fasta(rd[150:], 60),
        "crlf": _fasta(rd, 60).replace(b"\n", b"\r\n"),
        "nul_byte": _fasta(rd[:200], 60) + b">nul\nACGTACGTACGTACGTACGTACGTACG\0TACGTACGTACGTACGTACGTACGTACGTACGT\n" + _fasta(rd[200:], 60),
        "fastq_tail": _fasta(rd[:180], 60) + _fastq(rd[180:]),
        "truncated_in_last_line": _fasta(rd, 60)[:-17],
        "header_only_at_the_end": _fasta(rd, 60) + b">last",
    }
    return c


@pytest.fixture(scope="module")
def graph_ctx():
    cohort = get_cohort("cohort_snp")
    g = host.Graph(os.path.join(cohort.dir, "graph.bin.gz"))
    ctx = vgmi.Context(0, buffer_mib=16)
    g.upload(ctx)
    yield g, ctx, cohort
    ctx.close()
    g.close()


def _count(g, ctx, paths, monkeypatch, host_parse=False, chunk_kb=None, env=None):
    with monkeypatch.context() as m:
        m.setenv("VGH_HOST_PARSE", "1" if host_parse else "0")
        if chunk_kb:
            m.setenv("VGMI_FASTQ_CHUNK_KB", str(chunk_kb))
        else:
            m.delenv("VGMI_FASTQ_CHUNK_KB", raising=False)
        for k, v in (env or {}).items():
            m.setenv(k, v)
        cov, node, hist, st = g.sample_count(ctx, [str(p) for p in paths], threads=4, require_depth=False)
    return {"cov": cov, "node": node, "hist": hist, "n_reads": st["n_reads"], "read_base": st["read_base"]}


def _same(a, b, what=None):
    assert np.array_equal(a["cov"], b["cov"]) and np.array_equal(a["node"], b["node"]) and np.array_equal(a["hist"], b["hist"]), what
    assert (a["n_reads"], a["read_base"]) == (b["n_reads"], b["read_base"]), what


@pytest.mark.parametrize("name", sorted(_cases()))
def test_device_path_equals_host_reader(name, graph_ctx, tmp_path, monkeypatch):
    """Graph.sample_count on every input shape: the device path gives the host reader's counters, read_base and n_reads -- or its
    error -- whole and with 4, 5 and 64 KiB chunks; the host reader's counters are the oracle's on the block it returns."""
    g, ctx, cohort = graph_ctx
    p = tmp_path / "x.fa"
    p.write_bytes(_cases()[name])
    try:
        want = _count(g, ctx, [p], monkeypatch, host_parse=True)
    except vgmi.VgmiError as e:   # the reference aborts on this input (empty read): so must the device path, with the same message
        assert name in ("empty_record_in_the_middle", "header_only_at_the_end") and "empty read" in str(e)
        for chunk_kb in (None, 4, 5, 64):
            with pytest.raises(vgmi.VgmiError) as e2:
                _count(g, ctx, [p], monkeypatch, chunk_kb=chunk_kb)
            assert str(e2.value) == str(e)
        return
    assert name != "empty_record_in_the_middle"
    block, _n, rb = host.fastx_read_all(str(p))
    t = o.Table(cohort.graph.keys)
    if len(block):
        t.count_block(block, cohort.k)
    assert np.array_equal(want["cov"], t.counts())
    assert want["read_base"] == rb and want["n_reads"] == _n
    for chunk_kb in (None, 4, 5, 64):
        _same(_count(g, ctx, [p], monkeypatch, chunk_kb=chunk_kb), want, (name, chunk_kb))
    _same(_count(g, ctx, [p], monkeypatch, env={"VGH_DEVICE_FASTA": "0"}), want, (name, "today's path"))


def _header_offsets(text):
    """offsets of the header lines of a regular FASTA text (lines starting with '>')"""
    offs, p = [], 0
    for line in text.split(b"\n"):
        if line[:1] == b">":
            offs.append(p)
        p += len(line) + 1
    return offs


@pytest.mark.parametrize("width", [None, 60, "ragged"])
@pytest.mark.parametrize("piece", [None, 777, 4096])
def test_the_device_parses_fasta(width, piece, graph_ctx):
    """Ctx.fasta_text on a regular FASTA of n records: the device takes n - 1 of them (the last is complete only at the end of the
    data and comes back as the tail), and its counters are the oracle's on those reads."""
    g, ctx, cohort = graph_ctx
    rd = _reads(400, 7)
    text = _fasta(rd, width, seed=3)
    offs = _header_offsets(text)
    assert len(offs) == len(rd)
    ctx.counts_reset()
    r = ctx.fasta_text(text, piece=piece)
    cov, _, _ = ctx.counts_finish()
    assert not r["stopped"]
    assert (r["n_records"], r["n_bases"], r["consumed"]) == (len(rd) - 1, sum(map(len, rd[:-1])), offs[-1])
    assert r["tail"] == text[offs[-1]:]
    t = o.Table(cohort.graph.keys)
    t.count_block(np.frombuffer(b"".join(x + b"\n" for x in rd[:-1]), dtype=np.uint8), cohort.k)
    assert np.array_equal(cov, t.counts())


@pytest.mark.parametrize("chunk_kb", [None, 4])
def test_the_device_stops_at_the_record_with_a_plus_line(chunk_kb, graph_ctx, monkeypatch):
    g, ctx, _ = graph_ctx
    rd = _reads(300, 8)
    j = 123
    text = _fasta(rd[:j], 60) + b">bad\n" + rd[j][:20] + b"\n+\n" + rd[j][20:] + b"\n" + _fasta(rd[j + 1:], 60)
    with monkeypatch.context() as m:
        if chunk_kb:
            m.setenv("VGMI_FASTQ_CHUNK_KB", str(chunk_kb))
        ctx.counts_reset()
        r = ctx.fasta_text(text)
        ctx.counts_finish()
    assert (r["n_records"], r["n_bases"], r["consumed"], r["stopped"], r["tail"]) == (j, sum(map(len, rd[:j])), len(_fasta(rd[:j], 60)), True, b"")


def test_a_stream_that_is_not_fasta_is_handed_over_whole(graph_ctx):
    """vgmi_fastq_open_fasta on text that does not start with a header line: nothing is taken, the host reader has it all."""
    g, ctx, _ = graph_ctx
    text = b"junk\n" + _fasta(_reads(20, 9), 60)
    ctx.counts_reset()
    r = ctx.fasta_text(text)
    ctx.counts_finish()
    assert (r["n_records"], r["consumed"], r["stopped"]) == (0, 0, True)


def _bgzf_bytes(tmp_path, text, name="c", level=6, block=0xff00):
    src, dst = tmp_path / (name + ".fa"), tmp_path / (name + ".fa.bgz")
    src.write_bytes(text)
    synth.bgzf_compress_file(str(src), str(dst), level=level, block=block)
    return dst


@pytest.mark.parametrize("chunk_kb,block", [(None, 0xff00), (64, 3000)])
def test_compressed_fasta_is_inflated_and_parsed_on_the_device(chunk_kb, block, graph_ctx, tmp_path, monkeypatch):
    """Ctx.fasta_bgzf / fasta_gzip on a regular wrapped file: every record but the last on the device, no member refused, no give-up."""
    g, ctx, cohort = graph_ctx
    rd = _reads(3000, 10)
    text = _fasta(rd, 70)
    offs = _header_offsets(text)
    want = (len(rd) - 1, sum(map(len, rd[:-1])), offs[-1], False, text[offs[-1]:])
    t = o.Table(cohort.graph.keys)
    t.count_block(np.frombuffer(b"".join(x + b"\n" for x in rd[:-1]), dtype=np.uint8), cohort.k)
    with monkeypatch.context() as m:
        if chunk_kb:
            m.setenv("VGMI_FASTQ_CHUNK_KB", str(chunk_kb))
        ctx.counts_reset()
        r = ctx.fasta_bgzf(_bgzf_bytes(tmp_path, text, block=block).read_bytes())
        cov, _, _ = ctx.counts_finish()
        assert not r["inflate_failed"] and r["taken"] == os.path.getsize(tmp_path / "c.fa.bgz")
        assert (r["n_records"], r["n_bases"], r["consumed"], r["stopped"], r["tail"]) == want
        assert np.array_equal(cov, t.counts())
    if chunk_kb is None:
        ctx.counts_reset()
        r = ctx.fasta_gzip(gzip.compress(text, 6))
        cov, _, _ = ctx.counts_finish()
        assert r["stop"] == 1 and r["reason"] == 0 and r["device_text_bytes"] == len(text)
        assert (r["n_records"], r["n_bases"], r["consumed"], r["stopped"], r["tail"]) == want
        assert np.array_equal(cov, t.counts())


@pytest.fixture(scope="module")
def k22():
    cohort = get_cohort("cohort_k22")
    g = host.Graph(os.path.join(cohort.dir, "graph.bin.gz"))
    ctx = vgmi.Context(0, buffer_mib=16)
    g.upload(ctx)
    yield g, ctx, cohort
    ctx.close()
    g.close()


@pytest.fixture(scope="module")
def k21(tmp_path_factory):
    """a graph of another odd k, built by `varigraph-mi construct -k 21`"""
    import test_gpu_configs as cfg
    cfg._need_binaries()
    work = str(tmp_path_factory.mktemp("fasta_k21"))
    ref = synth.make_reference(80_000)
    variants, gts = synth.make_cohort(ref, 150, n_samples=4, ploidy=2, seed=5)
    fa, vcf, graph = os.path.join(work, "ref.fa"), os.path.join(work, "in.vcf"), os.path.join(work, "graph.bin")
    synth.write_fasta(fa, "chr1", ref)
    synth.write_vcf(vcf, "chr1", len(ref), variants, gts, 4, 2)
    r = cfg._run([cfg.CLI, "construct", "-r", fa, "-v", vcf, "--save-graph", graph, "-t", "16", "--gpu", "0", "-k", "21"], cwd=work,
                 capture_output=True, text=True, env=cfg.ENV, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    g = host.Graph(graph)
    ctx = vgmi.Context(0, buffer_mib=16)
    g.upload(ctx)
    hap = synth.sample_haplotypes(ref, variants, gts, 0, 2)[0]
    yield g, ctx, hap
    ctx.close()
    g.close()
    shutil.rmtree(work, ignore_errors=True)


@pytest.mark.parametrize("which", ["k27", "k21", "k22"])
def test_containers_through_the_product_path(which, request, tmp_path, monkeypatch):
    """The same FASTA text plain, gzip and block gzip: equal counters and stats, equal to the host reader's (k = 27 and 21 on the
    device, k = 22 through the host path)."""
    if which == "k27":
        g, ctx, cohort = request.getfixturevalue("graph_ctx")
        hap = cohort.haplotypes()[1]
    elif which == "k22":
        g, ctx, cohort = request.getfixturevalue("k22")
        hap = cohort.haplotypes()[1]
    else:
        g, ctx, hap = request.getfixturevalue("k21")
    rd = _reads(5000, 12, hap=hap)
    text = _fasta(rd, 80)
    plain, gz = tmp_path / "r.fa", tmp_path / "r.fa.gz"
    plain.write_bytes(text)
    with gzip.open(gz, "wb", compresslevel=4) as f:
        f.write(text)
    bgz = _bgzf_bytes(tmp_path, text, name="b")
    want = _count(g, ctx, [plain], monkeypatch, host_parse=True)
    assert (want["n_reads"], want["read_base"]) == (len(rd), sum(map(len, rd)))
    for p in (plain, gz, bgz):
        for chunk_kb in (None, 64):
            _same(_count(g, ctx, [p], monkeypatch, chunk_kb=chunk_kb), want, (which, p.name, chunk_kb))


def test_cli_genotype_on_fasta_equals_the_reference(tmp_path_factory):
    """`varigraph-mi genotype --use-depth` on a samples.cfg naming a wrapped .fa.gz, and one naming a FASTA and a FASTQ file of the
    same sample: the VCF the reference writes on the same files, byte for byte, with the device FASTA parser and without it."""
    import test_gpu_configs as cfg
    cfg._need_binaries()
    work = str(tmp_path_factory.mktemp("fasta_cli"))
    try:
        ref, variants, gts, graph = cfg._dataset(work, 200_000, 300, 5, 2)
        haps = synth.sample_haplotypes(ref, variants, gts, 0, 2)
        reads = vgmi.synth_reads_host(78, 0, 60_000, 150, haps).tobytes().split(b"\n")[:-1]
        half = len(reads) // 2
        fa_gz, fa, fq = os.path.join(work, "s.fa.gz"), os.path.join(work, "a.fasta"), os.path.join(work, "b.fq")
        with gzip.open(fa_gz, "wb", compresslevel=4) as f:
            f.write(_fasta(reads, 60))
        open(fa, "wb").write(_fasta(reads[:half], 70))
        open(fq, "wb").write(_fastq(reads[half:]))
        for tag, cfg_text in (("gz", f"sample0 {fa_gz}\n"), ("mix", f"sample0 {fa} {fq}\n")):
            cfg._reference_genotype(os.path.join(work, "cpu_" + tag), graph, cfg_text, ["--use-depth"], threads=10, timeout=300)
            want = cfg._vcf(os.path.join(work, "cpu_" + tag), "sample0")
            assert want.count(b"\n") > 100
            for dev in ("1", "0"):
                d = os.path.join(work, f"native_{tag}_{dev}")
                cfg._native_genotype(d, graph, cfg_text, ["--gpu", "0", "--use-depth"], threads=10, env={"VGH_DEVICE_FASTA": dev})
                assert cfg._vcf(d, "sample0") == want, (tag, dev)
    finally:
        shutil.rmtree(work, ignore_errors=True)


def test_long_records_on_the_device_and_beyond_the_carry(graph_ctx):
    """A 200 kb record wrapped at 80 is joined on the device; a 3 MiB one (longer than the 1 MiB carry) stops it at that record's header."""
    g, ctx, _ = graph_ctx
    rd = _reads(200, 13)
    front, back = _fasta(rd[:100], 80), _fasta(rd[100:], 80)
    text = front + _record(1000, _long_read(200_000), 80) + back
    ctx.counts_reset()
    r = ctx.fasta_text(text)
    ctx.counts_finish()
    assert (r["n_records"], r["n_bases"], r["stopped"]) == (len(rd), sum(map(len, rd[:-1])) + 200_000, False)
    ctx.counts_reset()
    r = ctx.fasta_text(front + _record(1000, _long_read(3 << 20), 80) + back)
    ctx.counts_finish()
    assert (r["n_records"], r["n_bases"], r["consumed"], r["stopped"], r["tail"]) == (100, sum(map(len, rd[:100])), len(front), True, b"")
