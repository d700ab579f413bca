"""Even k behind the device-side readers, through the C ABI (vgmi_fastq_*): FASTQ text in chunks of every size, read blocks around the
count kernels' row geometry, FASTA, block gzip, ordinary gzip and BAM -- the read block, its length, the reads' offsets and their number
never leave the device (csrc/vgmi_readoff.hip, the DEV forms of seq_kernel and even_debit_kernel).  Expected counters are the oracle's
(the reference's literal state machine on the '\\n'-joined reads); the reads are even_k_cases.py's."""
import gzip

import numpy as np
import pytest

import bam_py as B
import even_k_cases as E
from varigraph_amd import synth, vgmi

pytestmark = pytest.mark.gpu

_ctx = {}


@pytest.fixture(scope="module", autouse=True)
def _close_contexts():
    yield
    for c in _ctx.values():
        c.close()
    _ctx.clear()


def _table(name):
    """(case, a context that holds its table); the context-table cases must be on the context table"""
    case = E.make(name)
    if name not in _ctx:
        c = vgmi.Context(0, buffer_mib=16)
        c.table_upload(case.keys, case.k)
        assert (c.ctable_info()["n_buckets"] > 0) == ("context-table" in name), name
        _ctx[name] = c
    return case, _ctx[name]


def _chunks(monkeypatch, chunk_kb):
    if chunk_kb:
        monkeypatch.setenv("VGMI_FASTQ_CHUNK_KB", str(chunk_kb))
    else:
        monkeypatch.delenv("VGMI_FASTQ_CHUNK_KB", raising=False)


def _equal(cov, want, what):
    bad = np.flatnonzero(cov != want)
    assert bad.size == 0, (what, int(bad.size), bad[:5], cov[bad[:5]], want[bad[:5]])


def test_fastq_open_takes_an_even_k_table():
    """vgmi_fastq_open refused a table of even k ("the device-side FASTQ parser serves odd k"); it opens now, and a stream that is
    given nothing counts nothing."""
    case, ctx = _table("k22-path-table")
    ctx.counts_reset()
    r = ctx.fastq_text(b"")
    cov, _, _ = ctx.counts_finish()
    assert (r["n_records"], r["n_bases"], r["stopped"]) == (0, 0, False)
    assert not cov.any()


@pytest.mark.parametrize("chunk_kb", [None, 64, 4])
@pytest.mark.parametrize("name", list(E.TABLES))
def test_fastq_text(name, chunk_kb, monkeypatch):
    """The whole read set as FASTQ text, in whole staging buffers and in chunks of 64 and 4 KiB (records, and the carried tail,
    straddle the chunks): the oracle's counters, the input's records and bases -- twice, with a reset in between (the saturation
    flags of the first pass must be gone)."""
    case, ctx = _table(name)
    assert (case.want == 255).any() and (case.want < 255).any()
    text = E.fastq(case.reads)
    _chunks(monkeypatch, chunk_kb)
    for rep in range(2):
        ctx.counts_reset()
        r = ctx.fastq_text(text)
        cov, _, _ = ctx.counts_finish()
        assert (r["n_records"], r["n_bases"], r["stopped"], r["tail"]) == (len(case.reads), sum(map(len, case.reads)), False, b""), (name, rep)
        _equal(cov, case.want, (name, chunk_kb, rep))


def _geometry_blocks(case):
    """name -> reads, by the size of the PACKED block (not the file): around 768-byte rows (context table) and pairs of 1 024-byte rows
    (path table), with reads that make the run counter lag in them"""
    k, sp, rc = case.k, case.specials, case.own_rc
    body = case.genome[300:400]
    lag = [sp[2], sp[0], sp[5], sp[7], sp[10]]
    near_start = body[:10] + b"N" + rc[0] + body[10:]                   # a non-base at packed offset 10
    # 6 154 = 3 * 2 048 + 10 = 8 * 768 + 10: both fast kernels' rows end 10 bytes in front of the block's end, so a non-base just in
    # front of the rows' end is the debit pass's and lies within 33 bytes of the true end (the staged capacity is 1 MiB and more)
    head = E.fit(case, [near_start] + lag, 6154 - 140)
    last = case.genome[500:500 + 139 - 22] + b"N" + (rc[1] + rc[2])[:21]          # ... at packed offset 6 154 - 23 = 6 131
    assert sum(len(r) + 1 for r in head) == 6154 - 140 and len(last) == 139
    return {
        "under_768": E.fit(case, lag[:2], 700),
        "768_to_2047": E.fit(case, lag, 1800),
        "exactly_2048": E.fit(case, lag, 2048),
        "2049": E.fit(case, lag, 2049),
        "exactly_768": E.fit(case, lag[:3], 768),
        "single_read": [sp[2]],
        "single_long_read": [(sp[2] + sp[3] + body) * 12],
        "non_base_near_both_ends": head + [last],
    }


@pytest.mark.parametrize("name", list(E.TABLES))
def test_block_sizes_around_the_row_geometry(name, monkeypatch):
    """Read blocks under one row, between a row and a pair of rows, of exactly 2 048 and of 2 049 bytes, of a single read, with a
    non-base below packed offset 32 and within 33 bytes of the block's true end; and a first chunk that holds no complete record (one
    read longer than a 4 KiB chunk), which counts nothing and does not fail."""
    case, ctx = _table(name)
    _chunks(monkeypatch, None)
    for what, reads in _geometry_blocks(case).items():
        want = E.expected(case, reads)
        assert want.any(), what
        ctx.counts_reset()
        r = ctx.fastq_text(E.fastq(reads))
        cov, _, _ = ctx.counts_finish()
        assert (r["n_records"], r["n_bases"], r["stopped"]) == (len(reads), sum(map(len, reads)), False), (name, what)
        _equal(cov, want, (name, what))
    _chunks(monkeypatch, 4)
    long_read = (case.specials[2] + case.genome[:700]) * 6              # ~5 KB of sequence: the first 4 KiB chunk ends inside it
    reads = [long_read] + case.specials[:20]
    want = E.expected(case, reads)
    ctx.counts_reset()
    r = ctx.fastq_text(E.fastq(reads))
    cov, _, _ = ctx.counts_finish()
    assert (r["n_records"], r["n_bases"], r["stopped"]) == (len(reads), sum(map(len, reads)), False), name
    _equal(cov, want, (name, "no complete record in the first chunk"))


def _bgzf(tmp_path, text, name):
    src, dst = tmp_path / (name + ".txt"), tmp_path / (name + ".bgz")
    src.write_bytes(text)
    synth.bgzf_compress_file(str(src), str(dst), level=4)
    return dst.read_bytes()


@pytest.mark.parametrize("name", ["k22-path-table", "k28-context-table"])
def test_other_containers(name, tmp_path, monkeypatch):
    """The same reads as FASTA wrapped at 60 (the device leaves the last record, which only the end of the data completes, to its
    caller), as block gzip, as ordinary gzip and as BAM (the 4-bit codes other than A C G T are its non-bases)."""
    case, ctx = _table(name)
    _chunks(monkeypatch, None)
    reads, n_bases = case.reads, sum(map(len, case.reads))
    # FASTA
    ctx.counts_reset()
    r = ctx.fasta_text(E.fasta(reads))
    cov, _, _ = ctx.counts_finish()
    assert (r["n_records"], r["n_bases"], r["stopped"]) == (len(reads) - 1, n_bases - len(reads[-1]), False)
    assert r["tail"] == E.fasta(reads)[-len(r["tail"]):] and r["tail"].startswith(b">r%d " % (len(reads) - 1))
    _equal(cov, E.expected(case, reads[:-1]), (name, "fasta"))
    # block gzip, in whole buffers and in 64 KiB chunks
    text = E.fastq(reads)
    comp = _bgzf(tmp_path, text, "q")
    for chunk_kb in (None, 64):
        _chunks(monkeypatch, chunk_kb)
        ctx.counts_reset()
        r = ctx.fastq_bgzf(comp)
        cov, _, _ = ctx.counts_finish()
        assert not r["inflate_failed"] and not r["stopped"] and r["taken"] == len(comp)
        assert (r["n_records"], r["n_bases"]) == (len(reads), n_bases)
        _equal(cov, case.want, (name, "bgzf", chunk_kb))
    _chunks(monkeypatch, None)
    # ordinary gzip
    ctx.counts_reset()
    text = E.fastq(reads, qual_seed=5)
    r = ctx.fastq_gzip(gzip.compress(text, 6))
    cov, _, _ = ctx.counts_finish()
    assert (r["stop"], r["reason"], r["device_text_bytes"]) == (1, 0, len(text))
    assert (r["n_records"], r["n_bases"], r["stopped"]) == (len(reads), n_bases, False)
    _equal(cov, case.want, (name, "gzip"))
    # BAM: upper case only, and its own letters for the non-bases
    other = [b"N", b"R", b"M", b"K"]
    bam_reads = [r.upper().replace(b".", b"Y").replace(b"N", other[i % 4]) for i, r in enumerate(reads)]
    recs = [B.Rec(b"r%d" % i, s, flag=4) for i, s in enumerate(bam_reads)]
    path = tmp_path / "s.bam"
    hlen, _ = B.write_bam(path, recs)
    block, n_kept, rb = B.reads_block(recs)
    assert n_kept == len(reads) and rb == n_bases
    want = E.expected(case, bam_reads)
    assert (want == 255).any() and (want < 255).any()
    for chunk_kb in (None, 64):
        _chunks(monkeypatch, chunk_kb)
        ctx.counts_reset()
        r = ctx.bam_bgzf(path.read_bytes(), hlen, 0)
        cov, _, _ = ctx.counts_finish()
        assert not r["stopped"] and not r["inflate_failed"] and r["tail"] == b""
        assert (r["n_records"], r["n_bases"]) == (n_kept, rb)
        _equal(cov, want, (name, "bam", chunk_kb))


@pytest.mark.parametrize("name", ["k22-path-table", "k22-context-table-by-id"])
def test_debit_list_overflow_is_walked_on_the_spot(name, monkeypatch):
    """The scan writes the positions of non-bases into 256 lists by workgroup number, 4 096 entries each (VG_DEBIT_LIST / VG_DEBIT_SUBLISTS),
    a workgroup per 16 KiB of text: 9 KiB of "NANA.." in the block's first 16 KiB are more non-bases with a base behind them than
    its list holds, so what the list refuses -- the lagging reads next to them among it -- is walked where the scan finds it."""
    case, ctx = _table(name)
    _chunks(monkeypatch, None)
    sp = case.specials
    lagging = [sp[i] for i in range(len(sp)) if i % 13 in (2, 4, 5, 6)]
    first_16k = []
    for i in range(60):
        first_16k += [b"NA" * 75, lagging[i % len(lagging)]]
    assert E.block_of(first_16k).size > 16384 and E.block_of(first_16k)[:16384].tobytes().count(b"N") > 4096 + 200
    reads = first_16k + case.reads[:600]
    want = E.expected(case, reads)
    ctx.counts_reset()
    r = ctx.fastq_text(E.fastq(reads))
    cov, _, _ = ctx.counts_finish()
    assert r["n_records"] == len(reads) and not r["stopped"]
    _equal(cov, want, name)
