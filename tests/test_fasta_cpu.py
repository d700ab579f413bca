"""What the FASTA device path shows without a device: the C entry is declared and exported, and the host side's decision which
parser a file goes to (vgh_sniff_input: container by magic, BAM / FASTA / other by the first bytes of the text)."""
import gzip
import os
import subprocess

import pytest

import bam_py as B
from varigraph_amd import host, synth, vgmi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_and_header_declares_the_fasta_entry():
    header = open(os.path.join(ROOT, "include", "vgmi.h")).read()
    assert "int vgmi_fastq_open_fasta(vgmi_ctx *ctx, vgmi_fastq **out);" in header
    lib = os.path.join(ROOT, "varigraph_amd", "libvgmi.so")
    assert os.path.exists(lib), "build first: python -m varigraph_amd.build"
    syms = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    assert any(line.split()[-1] == "vgmi_fastq_open_fasta" and line.split()[-2] == "T" for line in syms.splitlines() if line.strip())
    for name in ("fasta_text", "fasta_bgzf", "fasta_gzip"):
        assert callable(getattr(vgmi.Context, name))


_TEXTS = {
    "fasta": (b">r1 c\nACGT\nAC\n>r2\nGG\n", ord(">"), True),
    "fastq": (b"@r1\nACGT\n+\nIIII\n", ord("@"), False),
    "junk": (b"junk\n>r1\nACGT\n", ord("j"), False),
    "empty": (b"", -1, False),
}


def _write(tmp_path, kind, text):
    p = tmp_path / ("x." + kind)
    if kind == "plain":
        p.write_bytes(text)
    elif kind == "gzip":
        p.write_bytes(gzip.compress(text, 6))
    else:
        q = tmp_path / "x.txt"
        q.write_bytes(text)
        synth.bgzf_compress_file(str(q), str(p))
    return str(p)


@pytest.mark.parametrize("kind", ["plain", "gzip", "bgzf"])
@pytest.mark.parametrize("what", sorted(_TEXTS))
def test_sniffing(kind, what, tmp_path, monkeypatch):
    text, first, fasta = _TEXTS[what]
    p = _write(tmp_path, kind, text)
    monkeypatch.delenv("VGH_DEVICE_FASTA", raising=False)
    r = host.sniff_input(p)
    # (an empty plain file has no magic: plain; an empty text compressed is still its container)
    assert r == {"kind": kind, "first_byte": first, "bam": False, "fasta": fasta}
    monkeypatch.setenv("VGH_DEVICE_FASTA", "0")
    assert host.sniff_input(p) == {"kind": kind, "first_byte": first, "bam": False, "fasta": False}


def test_sniffing_a_bam_and_a_missing_file(tmp_path):
    p = tmp_path / "u.bam"
    B.write_bam(p, [B.Rec(b"r1", b"ACGTACGT", flag=4)])
    r = host.sniff_input(str(p))
    assert (r["kind"], r["bam"], r["fasta"], r["first_byte"]) == ("bgzf", True, False, ord("B"))
    with pytest.raises(RuntimeError, match="No such file or directory"):
        host.sniff_input(str(tmp_path / "absent.fa"))
