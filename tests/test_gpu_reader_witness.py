"""The read files of tests/reader_witness.py through the device FASTQ and FASTA parsers (csrc/vgmi_fastq.hip, csrc/vgmi_fasta.hip) by
the plain-text path of the C ABI (Context.fastq_text / fasta_text = vgmi_fastq_open[_fasta] + vgmi_fastq_commit), as each case cuts it
and again in one commit: records, bases, consumed bytes, the stop and the tail -- masked bases and reads numbered where they apply --
as the plain-Python model says, and the counters bit for bit against the oracle on the model's read block.  The key table holds every
k-mer of the genome the reads tile, so one byte the copy kernels drop, shift or garble changes a counter.  The two families in which
the device stops (a record longer than the carry, more lines than the arrays hold) also go through the product path
(Graph.sample_count): device and host reader together must count the whole file.  tests/test_reader_witness_cpu.py proves the cases
are what they claim."""
import numpy as np
import pytest

import oracle_lib as o
import reader_witness as W
from varigraph_amd import host, vgmi

pytestmark = pytest.mark.gpu


class _Device:
    """a context whose table holds every k-mer of the witness genome, and the oracle's table of the same keys"""

    def __init__(self, k):
        self.k, self.keys = k, W.keys(k)
        self.table = o.Table(self.keys)
        self.ctx = vgmi.Context(0, buffer_mib=W.STAGING_MIB)
        self.ctx.table_upload(self.keys, k)

    def want(self, block):
        self.table.reset()
        if block:
            self.table.count_block(np.frombuffer(block, dtype=np.uint8), self.k)
        return self.table.counts()

    def run(self, c, pieces):
        self.ctx.counts_reset()
        if c.kind == "fastq":
            r = self.ctx.fastq_text(c.text, piece=pieces, min_quality=c.min_quality, subsample=c.subsample)
        else:
            r = self.ctx.fasta_text(c.text, piece=pieces, subsample=c.subsample)
        return r, self.ctx.counts_finish()[0]


_DEVICES = {}


@pytest.fixture(scope="module")
def device():
    def get(k):
        if k not in _DEVICES:
            _DEVICES[k] = _Device(k)
        return _DEVICES[k]
    yield get
    for d in _DEVICES.values():
        d.ctx.close()
    _DEVICES.clear()


@pytest.fixture(scope="module")
def witness_graph(tmp_path_factory):
    p = tmp_path_factory.mktemp("witness") / "graph.bin"
    p.write_bytes(W.graph_bin(W.K))
    g = host.Graph(str(p))
    ctx = vgmi.Context(0, buffer_mib=W.STAGING_MIB)
    g.upload(ctx)
    yield g, ctx
    ctx.close()
    g.close()


def _env(m, c):
    m.delenv("VGMI_FASTQ_CHUNK_KB", raising=False)
    m.delenv("VGMI_FASTQ_TEXT_MB", raising=False)
    for key, v in c.env.items():
        m.setenv(key, v)


def _check(d, c, pieces, monkeypatch):
    want = W.model(c, pieces)
    with monkeypatch.context() as m:
        _env(m, c)
        r, cov = d.run(c, c.pieces if pieces == "as cut" else pieces)
    got = (r["n_records"], r["n_bases"], r["consumed"], r["stopped"], r["tail"])
    if c.min_quality:
        got += (r["masked_bases"],)
    if c.subsample:
        got += (r["n_seen"],)
    print(c.name, d.k, "%d commits" % len(want.ends), got[:4], len(got[4]), got[5:])
    assert got == want.report(c), (c.name, pieces)
    oracle = d.want(want.block)
    assert np.array_equal(cov, oracle), (c.name, pieces, int((cov != oracle).sum()))
    return cov


def _check_product(witness_graph, c, tmp_path, monkeypatch):
    """Graph.sample_count on the file, the device parser on: the oracle's counters on ALL reads of the file -- what the device took and
    what the host reader took over --, and their number and bases"""
    g, ctx = witness_graph
    p = tmp_path / (c.name + (".fq" if c.kind == "fastq" else ".fa"))
    p.write_bytes(c.file)
    reads, _, _ = W.whole(c)
    keys = g.arrays()["keys"]
    t = o.Table(keys)
    t.count_block(np.frombuffer(W.block_of(reads), dtype=np.uint8), W.K)
    with monkeypatch.context() as m:
        _env(m, c)
        m.setenv("VGH_HOST_PARSE", "0")
        cov, node, hist, st = g.sample_count(ctx, [str(p)], threads=4, require_depth=False)
    assert (st["n_reads"], st["read_base"]) == (len(reads), sum(map(len, reads))), c.name
    assert np.array_equal(cov, t.counts()), c.name


@pytest.mark.parametrize("k,name", [(k, n) for n in W.names() for k in W.get(n).tables])
def test_case(k, name, device, witness_graph, tmp_path, monkeypatch):
    c, d = W.get(name), device(k)
    cov = _check(d, c, "as cut", monkeypatch)
    if c.again_in_one_commit and c.pieces is not None:
        assert np.array_equal(_check(d, c, None, monkeypatch), cov)
    if c.family in ("carry", "line_cap"):
        _check_product(witness_graph, c, tmp_path, monkeypatch)
