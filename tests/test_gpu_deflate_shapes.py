"""The hand-built DEFLATE streams of tests/test_deflate_shapes_cpu.py through both device decoders -- vgmi_gunzip.hip (ordinary gzip:
ctx.gunzip, and the stream form fastq_gzip) and vgmi_inflate.hip (block gzip: fastq_bgzf) -- in both forms of their inner loop: wide
batches in this process, the first form (VGMI_INFLATE_WIDE=0, read once per process) in a child.  The contract is that of
test_gpu_gunzip.py: what the device hands back is a PREFIX of zlib's output, and all of it, with a clean member end, for every
stream zlib accepts (the two `trap` cases excepted, where a stretch is cut at a false block start and the host decoder takes over).

run_all() puts every case through the device and returns plain data (the child writes it as JSON); the check_* functions hold the
assertions and are applied to both forms' results."""
import base64
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
STREAM = ("short_literal_runs", "big_member", "distances_x_lengths")      # members of the stream-form run
PIECES = (None, 150_000)
LEAD = "short_literal_runs"                                               # the good member in front of every refused block-gzip member
BGZF_DATA = 18                                                            # a block-gzip member's header: its DEFLATE bytes start here


def _b64(b):
    return base64.b64encode(bytes(b)).decode()


def _keep(r):
    return {k: (_b64(v) if isinstance(v, bytes) else v) for k, v in r.items()}


_RESIDUES = None


def residue_members():
    """Eight block-gzip members -- FASTQ records around the blocks of stored_alignments (stored, fixed, dynamic) and dynamic_headers in
    turn -- whose DEFLATE bytes start at every residue mod 4 of the file offset: the device reads a member's input as aligned words
    from wherever it lies.  A character more in a record's name is a byte more of DEFLATE data (a fixed code of eight bits), so every
    member is given the name that makes its size 1 mod 4: each starts a residue behind the one before it.
    -> (the members, their texts, the kinds of block in them)"""
    global _RESIDUES
    if _RESIDUES is None:
        import deflate_builder as db
        import test_deflate_shapes_cpu as shapes
        members, texts, kinds = [], [], set()
        for i in range(8):
            inner = shapes._case_stored_alignments() if i % 2 == 0 else shapes._case_headers()
            for pad in range(4):
                blocks = shapes._record(inner, name=b"m%d" % i + b"x" * pad)
                text = shapes._tokens_text(blocks)
                m = db.bgzf_member(db.deflate(blocks), text)
                if len(m) % 4 == 1:
                    break
            members.append(m)
            texts.append(text)
            kinds |= {type(b).__name__ for b in blocks}
        _RESIDUES = members, texts, kinds
    return _RESIDUES


def run_all():
    import deflate_builder as db
    import test_deflate_shapes_cpu as shapes
    from conftest import get_cohort
    from varigraph_amd import host, vgmi
    cohort = get_cohort("cohort_snp")
    g = host.Graph(os.path.join(cohort.dir, "graph.bin.gz"))
    c = vgmi.Context(0, buffer_mib=16)
    g.upload(c)
    res = {"gzip": {}, "bgzf_bad": {}, "stream": []}
    try:
        cases = shapes.cases()
        for k in cases:
            if k.gzip:
                got, consumed, end, why = c.gunzip(k.gz(), len(k.text) + 70_000)
                res["gzip"][k.name] = {"got": _b64(got), "consumed": consumed, "end": end, "why": why}
        for key, fastq in (("bgzf_fastq", True), ("bgzf_other", False)):
            comp = b"".join(k.bz() for k in cases if k.ok and k.bgzf and k.fastq == fastq) + db.BGZF_EOF
            c.counts_reset()
            r = c.fastq_bgzf(comp)
            cov, _, _ = c.counts_finish()
            res[key] = dict(_keep(r), cov=_b64(cov.tobytes()))
        c.counts_reset()
        r = c.fastq_bgzf(b"".join(residue_members()[0]) + db.BGZF_EOF)
        cov, _, _ = c.counts_finish()
        res["bgzf_residues"] = dict(_keep(r), cov=_b64(cov.tobytes()))
        lead = shapes.by_name(LEAD).bz()
        for k in cases:
            if not k.ok and k.bgzf:
                c.counts_reset()
                r = c.fastq_bgzf(lead + k.bz() + lead + db.BGZF_EOF)
                c.counts_finish()
                res["bgzf_bad"][k.name] = _keep(r)
        comp = b"".join(shapes.by_name(n).gz() for n in STREAM)
        for piece in PIECES:
            c.counts_reset()
            r = c.fastq_gzip(comp, piece=piece)
            cov, _, _ = c.counts_finish()
            res["stream"].append(dict(_keep(r), cov=_b64(cov.tobytes())))
    finally:
        c.close()
        g.close()
    return res


def _counts(texts):
    import oracle_lib as o
    from conftest import get_cohort
    cohort = get_cohort("cohort_snp")
    reads = [ln for t in texts for ln in t.split(b"\n")[1::4]]
    t = o.Table(cohort.graph.keys)
    t.count_block(np.frombuffer(b"".join(r + b"\n" for r in reads), dtype=np.uint8), cohort.k)
    return len(reads), t.counts()


_WANT = {}


def _want(key, names):
    """(records, counters of the oracle) of the named cases' texts run together: computed once, shared by both forms"""
    import test_deflate_shapes_cpu as shapes
    if key not in _WANT:
        _WANT[key] = _counts([shapes.by_name(n).text for n in names])
    return _WANT[key]


def check_gzip(res):
    import test_deflate_shapes_cpu as shapes
    ran = 0
    for k in shapes.cases():
        if not k.gzip:
            continue
        r = res["gzip"][k.name]
        got = base64.b64decode(r["got"])
        print(k.name, "ok" if k.ok else "refused", len(k.body), len(k.text), "->", len(got), r["consumed"], r["end"], r["why"])
        if k.must:
            assert (r["end"], r["why"]) == (True, 0), (k.name, r["end"], r["why"], len(got), len(k.text))
            assert got == k.text, k.name
            assert r["consumed"] == len(k.gz()) - 8, k.name
        else:
            assert got == k.text[:len(got)], (k.name, len(got))
            if not k.ok:
                assert not (r["end"] and r["why"] == 0), k.name       # never a clean member end where zlib raised (or ran out of input)
            elif r["end"]:
                assert got == k.text and r["why"] == 0, k.name
        ran += 1
    assert ran >= 45


def check_bgzf(res):
    import deflate_builder as db
    import test_deflate_shapes_cpu as shapes
    cases = shapes.cases()
    fq = [k for k in cases if k.ok and k.bgzf and k.fastq]
    other = [k for k in cases if k.ok and k.bgzf and not k.fastq]
    assert len(fq) >= 9 and {"dense_matches", "long_codes", "all_symbols_fixed"} <= {k.name for k in fq} and len(other) >= 3
    r = res["bgzf_fastq"]
    total = sum(len(k.bz()) for k in fq) + len(db.BGZF_EOF)
    n_rec, want = _want("bgzf", [k.name for k in fq])
    assert not r["inflate_failed"] and not r["stopped"], (r["reason"], r["good_compressed_bytes"])
    assert r["taken"] == r["good_compressed_bytes"] == total
    assert r["consumed"] == sum(len(k.text) for k in fq) and r["n_records"] == n_rec and base64.b64decode(r["tail"]) == b""
    assert np.array_equal(np.frombuffer(base64.b64decode(r["cov"]), dtype=np.uint8), want) and want.any()
    # text that is no FASTQ: the parser hands it over, the members are inflated all the same -- their CRC-32 is checked on the device
    r = res["bgzf_other"]
    assert not r["inflate_failed"] and r["good_compressed_bytes"] == sum(len(k.bz()) for k in other) + len(db.BGZF_EOF), (r["reason"], r["good_compressed_bytes"])
    # a member zlib refuses: named by its compressed offset, nothing behind it parsed
    lead = shapes.by_name(LEAD)
    bad = [k for k in cases if not k.ok and k.bgzf]
    assert len(bad) >= 29
    for k in bad:
        r = res["bgzf_bad"][k.name]
        assert r["inflate_failed"] and r["good_compressed_bytes"] == len(lead.bz()), (k.name, r["inflate_failed"], r["good_compressed_bytes"], r["reason"])
        assert r["consumed"] + len(base64.b64decode(r["tail"])) == len(lead.text) and r["n_records"] <= 1, k.name


def check_residues(res):
    import deflate_builder as db
    import zlib
    members, texts, kinds = residue_members()
    # where every member's DEFLATE bytes start in the file, from the sizes written
    starts = [sum(len(m) for m in members[:i]) + BGZF_DATA for i in range(len(members))]
    assert len(members) >= 8 and {s % 4 for s in starts} == {0, 1, 2, 3}, starts
    assert kinds == {"Stored", "Fixed", "Dynamic"}
    for m, t in zip(members, texts):
        assert zlib.decompressobj(-15).decompress(m[BGZF_DATA:-8]) == t
    assert sum(len(t) for t in texts) < 16384
    r = res["bgzf_residues"]
    total = sum(len(m) for m in members) + len(db.BGZF_EOF)
    if "residues" not in _WANT:
        _WANT["residues"] = _counts(texts)
    n_rec, want = _WANT["residues"]
    assert not r["inflate_failed"] and not r["stopped"], (r["reason"], r["good_compressed_bytes"])
    assert r["taken"] == r["good_compressed_bytes"] == total
    assert r["consumed"] == sum(len(t) for t in texts) and r["n_records"] == n_rec == len(members) and base64.b64decode(r["tail"]) == b""
    assert np.array_equal(np.frombuffer(base64.b64decode(r["cov"]), dtype=np.uint8), want) and want.any()


def check_stream(res):
    import test_deflate_shapes_cpu as shapes
    n_rec, want = _want("stream", STREAM)
    n_text = sum(len(shapes.by_name(n).text) for n in STREAM)
    n_comp = sum(len(shapes.by_name(n).gz()) for n in STREAM)
    assert len(res["stream"]) == len(PIECES)
    for piece, r in zip(PIECES, res["stream"]):
        assert (r["stop"], r["reason"], r["stopped"]) == (1, 0, False), (piece, r["stop"], r["reason"])
        assert r["device_text_bytes"] == n_text and r["taken"] == n_comp, piece
        assert (r["n_records"], r["consumed"], base64.b64decode(r["tail"])) == (n_rec, n_text, b""), piece
        assert np.array_equal(np.frombuffer(base64.b64decode(r["cov"]), dtype=np.uint8), want), piece


@pytest.fixture(scope="module")
def wide():
    assert os.environ.get("VGMI_INFLATE_WIDE", "1")[:1] != "0"
    return run_all()


@pytest.fixture(scope="module")
def first_form(tmp_path_factory):
    """the same list in a fresh process with VGMI_INFLATE_WIDE=0, run once"""
    out = str(tmp_path_factory.mktemp("first_form") / "results.json")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), out], env=dict(os.environ, VGMI_INFLATE_WIDE="0"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    with open(out) as f:
        return json.load(f)


def test_ordinary_gzip_wide(wide):
    check_gzip(wide)


def test_block_gzip_wide(wide):
    check_bgzf(wide)


def test_block_gzip_members_at_every_alignment_wide(wide):
    check_residues(wide)


def test_gzip_stream_wide(wide):
    check_stream(wide)


def test_ordinary_gzip_first_form(first_form):
    check_gzip(first_form)


def test_block_gzip_first_form(first_form):
    check_bgzf(first_form)


def test_block_gzip_members_at_every_alignment_first_form(first_form):
    check_residues(first_form)


def test_gzip_stream_first_form(first_form):
    check_stream(first_form)


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(HERE))
    sys.path.insert(0, HERE)
    assert os.environ.get("VGMI_INFLATE_WIDE") == "0"
    with open(sys.argv[1], "w") as f:
        json.dump(run_all(), f)
