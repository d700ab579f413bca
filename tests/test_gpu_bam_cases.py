"""The hand-built BAM streams of tests/bam_cases.py through the device's record kernels (csrc/vgmi_bam.hip) by the C ABI
(Context.bam_bgzf = vgmi_fastq_open_bam + vgmi_fastq_commit_bgzf), chunk by chunk as each case cuts it and again in one commit:
records, bases, consumed bytes, the stop and the tail as the Python model says, and the counters bit for bit against the oracle on
the model's read block.  The key table holds the k-mers of every sequence in the cases -- true records and planted fakes alike -- so
one wrongly decoded base, or a chain that enters a fake, changes a counter.  Where the device stops, the product path
(Graph.sample_count) must give what the host decoder gives: the same counters, or the same error naming the same byte.
tests/test_bam_cases_cpu.py proves the cases are what they claim."""
import os

import numpy as np
import pytest

import bam_cases as K
import oracle_lib as o
from conftest import get_cohort
from varigraph_amd import host, vgmi

pytestmark = pytest.mark.gpu

_SHORT = ["seqlen_k11"] + K.names("chain") + [n for n in K.names("sweep") if n.startswith("header")]
_EVEN = ["seqlen_k22", "binary_search_6_fakes", "fakes_in_the_carried_tail", "sweep_m2_fakes"]
RUNS = {27: [n for n in K.names() if n not in ("seqlen_k11", "seqlen_k22")], 11: _SHORT, 22: _EVEN}
CAPACITY = K.names("capacity")[0]


class _Device:
    """a context whose table holds the k-mers of every sequence of the cases run at k, and the oracle's table of the same keys"""

    def __init__(self, k):
        self.k = k
        keys = [o.sketch(r, k) for n in RUNS[k] for r in K.get(n).reads if len(r) >= k]
        keys = np.unique(np.concatenate(keys))
        self.keys = keys[keys != np.uint64(0xFFFFFFFFFFFFFFFF)]
        self.table = o.Table(self.keys)
        self.ctx = vgmi.Context(0, buffer_mib=16)
        self.ctx.table_upload(self.keys, k)

    def want(self, block):
        self.table.reset()
        if block:
            self.table.count_block(np.frombuffer(block, dtype=np.uint8), self.k)
        return self.table.counts()

    def run(self, c, piece):
        self.ctx.counts_reset()
        r = self.ctx.bam_bgzf(c.comp, c.hlen, c.n_ref, piece=piece)
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
def snp():
    cohort = get_cohort("cohort_snp")
    g = host.Graph(os.path.join(cohort.dir, "graph.bin.gz"))
    ctx = vgmi.Context(0, buffer_mib=16)
    g.upload(ctx)
    yield g, ctx
    ctx.close()
    g.close()


def _check(d, c, piece):
    r, cov = d.run(c, piece)
    got = (r["n_records"], r["n_bases"], r["consumed"], r["stopped"], r["tail"], r["inflate_failed"])
    print(c.name, d.k, "one commit" if piece is None else "%d commits" % len(piece), got[:4], len(r["tail"]))
    assert got == (c.n_records, c.n_bases, c.consumed, c.stopped, c.tail, False), (c.name, piece)
    assert r["taken"] == len(c.comp)
    assert np.array_equal(cov, d.want(c.block)), (c.name, piece)
    return cov


def _product(g, ctx, path, monkeypatch, host_parse, env):
    with monkeypatch.context() as m:
        m.setenv("VGH_HOST_PARSE", "1" if host_parse else "0")
        m.delenv("VGMI_FASTQ_CHUNK_KB", raising=False)
        for key, v in env.items():
            m.setenv(key, v)
        try:
            cov, node, hist, st = g.sample_count(ctx, [str(path)], threads=4, require_depth=False)
        except vgmi.VgmiError as e:
            return str(e)
    return cov.tobytes(), node.tobytes(), hist.tobytes(), st["n_reads"], st["read_base"]


def _check_product(snp, c, tmp_path, monkeypatch):
    """the device path and the host decoder on the file: the same counters, or the same error naming the same byte"""
    g, ctx = snp
    p = tmp_path / (c.name + ".bam")
    p.write_bytes(c.comp)
    want, got = _product(g, ctx, p, monkeypatch, True, c.env), _product(g, ctx, p, monkeypatch, False, c.env)
    assert got == want, c.name
    if c.error_what:
        assert isinstance(want, str) and c.error(p) in want, want
    else:
        reads = [r.seq for r in c.recs if r.kept]
        assert want[3:] == (len(reads), sum(map(len, reads)))


@pytest.mark.parametrize("k,name", [(k, n) for k in RUNS for n in RUNS[k] if n != CAPACITY])
def test_case(k, name, device, snp, tmp_path, monkeypatch):
    c, d = K.get(name), device(k)
    cov = _check(d, c, c.piece)
    assert np.array_equal(_check(d, c, None), cov)
    if k == 27 and (c.stop is not None or c.family == "carry"):
        _check_product(snp, c, tmp_path, monkeypatch)


def test_a_fake_entered_would_show(device):
    """the table holds the planted fakes' k-mers: the wrong walk's read block gives other counters than the true one"""
    d, c = device(27), K.get("binary_search_6_fakes")
    off, _, fake = c.fakes[0]
    wrong, n, _ = K.walk(c.raw, off, len(c.raw), c.n_ref)
    assert n >= 1 and not np.array_equal(d.want(c.block + wrong), d.want(c.block)) and d.want(c.block).any()


def test_more_candidates_than_the_arrays_hold(device, snp, tmp_path, monkeypatch):
    """Chunks of 64 KiB (VGMI_FASTQ_CHUNK_KB) carry the front of a record whose aux array is a candidate every 16 bytes: when they exceed
    the candidate arrays the device takes nothing of the chunk and stops at the carried record's first byte; the host decodes the rest."""
    c, d = K.get(CAPACITY), device(27)
    with monkeypatch.context() as m:
        for key, v in c.env.items():
            m.setenv(key, v)
        r, cov = d.run(c, None)
    print(c.name, r["n_records"], r["n_bases"], r["consumed"], r["stopped"], len(r["tail"]))
    assert (r["n_records"], r["n_bases"], r["consumed"], r["stopped"], r["tail"], r["inflate_failed"]) == \
        (c.n_records, c.n_bases, c.consumed, True, b"", False)
    assert np.array_equal(cov, d.want(c.block))
    _check_product(snp, c, tmp_path, monkeypatch)
