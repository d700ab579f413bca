"""bench_fasta.py -- a sample's reads through vgh_sample_count as FASTA on the device parser (vgmi_fasta.hip), next to (a) the FASTQ
twin of the same reads on the device FASTQ parser and (b) the same FASTA file on the path it took before (VGH_DEVICE_FASTA=0: the
FASTQ-mode parser stops at record 0 and the host reader takes the file), alternating in one process, median of --reps.

    python tools/bench_fasta.py [--reads 20000000] [--reps 3] [--dir DIR] [--only short|hifi] [--container plain|bgzf]
                                [--out profiles/fasta_bench.json]

Two read sets of the same number of bases, drawn from the C1 cohort's haplotypes (tests/golden/c1; seeded):
  short  --reads reads of 150 bases, one sequence line each
  hifi   reads of 15 000 bases wrapped at 80 columns
each as a plain file and as block gzip (members of 0xff00 bytes of text).  Prints one JSON line and writes it to --out."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from varigraph_amd import host, synth, vgmi  # noqa: E402
from bench_bam import BgzfWriter  # noqa: E402

WIDTH = 80
PIECE_BASES = 150_000_000     # bases generated and laid out at a time
SETS = {"short": (150, None), "hifi": (15_000, WIDTH)}


class PlainWriter:
    def __init__(self, path):
        self.f = open(path, "wb")

    def write(self, data):
        self.f.write(data)

    def close(self):
        self.f.close()


def _names(m, idx, lead):
    """'<lead>r%09d\\n' into the first 12 columns of m"""
    m[:, 0], m[:, 1] = ord(lead), ord("r")
    for d in range(9):
        m[:, 2 + d] = (idx // 10 ** (8 - d)) % 10 + ord("0")
    m[:, 11] = 10


def _fasta(rows, first, width):
    n, L = rows.shape
    idx = np.arange(first, first + n, dtype=np.int64)
    if width is None:
        m = np.empty((n, 12 + L + 1), dtype=np.uint8)
        _names(m, idx, ">")
        m[:, 12:12 + L] = rows
        m[:, 12 + L] = 10
        return m
    full, rest = L // width, L % width
    m = np.empty((n, 12 + full * (width + 1) + (rest + 1 if rest else 0)), dtype=np.uint8)
    _names(m, idx, ">")
    body = m[:, 12:12 + full * (width + 1)].reshape(n, full, width + 1)
    body[:, :, :width] = rows[:, :full * width].reshape(n, full, width)
    body[:, :, width] = 10
    if rest:
        m[:, -rest - 1:-1] = rows[:, full * width:]
        m[:, -1] = 10
    return m


def _fastq(rows, first):
    n, L = rows.shape
    m = np.empty((n, 12 + L + 3 + L + 1), dtype=np.uint8)
    _names(m, np.arange(first, first + n, dtype=np.int64), "@")
    m[:, 12:12 + L] = rows
    m[:, 12 + L], m[:, 13 + L], m[:, 14 + L] = 10, ord("+"), 10
    m[:, 15 + L:15 + 2 * L] = ord("?")
    m[:, 15 + 2 * L] = 10
    return m


def _draw(first, n, L, haps):
    """n reads of L bases as an n x L array: the seeded generator's up to its longest read (350), windows of the haplotypes beyond"""
    if L <= 350:
        return vgmi.synth_reads_host(4242, first, n, L, haps).reshape(n, L + 1)[:, :L]
    rng = np.random.default_rng([4242, first])
    rows = np.empty((n, L), dtype=np.uint8)
    which = rng.integers(0, len(haps), size=n)
    for h, hap in enumerate(haps):
        sel = np.flatnonzero(which == h)
        starts = rng.integers(0, hap.size - L, size=sel.size)
        rows[sel] = hap[starts[:, None] + np.arange(L, dtype=np.int64)[None, :]]
    return rows


def make_files(d, n_reads, L, width, haps, bgzf, level):
    ext = ".gz" if bgzf else ""
    fa, fq = os.path.join(d, "reads.fa" + ext), os.path.join(d, "reads.fq" + ext)
    piece = max(1, (PIECE_BASES if L <= 350 else PIECE_BASES // 5) // L)
    with ThreadPoolExecutor(16) as pool:
        wa, wq = (BgzfWriter(fa, level, pool), BgzfWriter(fq, level, pool)) if bgzf else (PlainWriter(fa), PlainWriter(fq))
        for first in range(0, n_reads, piece):
            n = min(piece, n_reads - first)
            rows = _draw(first, n, L, haps)
            wa.write(_fasta(rows, first, width).tobytes())
            wq.write(_fastq(rows, first).tobytes())
        wa.close()
        wq.close()
    return fa, fq


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=20_000_000, help="reads of the short set; the hifi set has the same number of bases")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--level", type=int, default=1)
    ap.add_argument("--dir", default=None)
    ap.add_argument("--only", choices=sorted(SETS), default=None)
    ap.add_argument("--container", choices=["plain", "bgzf"], default=None)
    ap.add_argument("--skip-today", action="store_true", help="profiling runs: without the VGH_DEVICE_FASTA=0 leg")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fasta_bench.json"))
    a = ap.parse_args()
    gdir = os.path.join(ROOT, "tests", "golden", "c1")
    meta = json.load(open(os.path.join(gdir, "meta.json")))
    ref = synth.make_reference(meta["ref_len"], seed=meta["ref_seed"])
    variants, gts = synth.make_cohort(ref, meta["n_var"], n_samples=meta["n_samples"], ploidy=meta["ploidy"], seed=meta["cohort_seed"])
    haps = synth.sample_haplotypes(ref, variants, gts, 0, meta["ploidy"])
    g = host.Graph(os.path.join(gdir, "graph.bin.gz"))
    ctx = vgmi.Context(0)
    g.upload(ctx)
    os.environ.pop("VGH_DEVICE_FASTA", None)
    files = {}
    for name in ([a.only] if a.only else sorted(SETS, reverse=True)):
        L, width = SETS[name]
        n_reads = max(2, a.reads * 150 // L)
        for bgzf in ((False, True) if a.container is None else (a.container == "bgzf",)):
            tmp = tempfile.TemporaryDirectory(dir=a.dir)
            t0 = time.perf_counter()
            fa, fq = make_files(tmp.name, n_reads, L, width, haps, bgzf, a.level)
            t_make = time.perf_counter() - t0
            legs = {"fasta": (fa, None), "fastq_twin": (fq, None), "fasta_today": (fa, "0")}
            if a.skip_today:
                del legs["fasta_today"]
            rates, stats = {k: [] for k in legs}, {}
            g.sample_count(ctx, [fa], threads=16, require_depth=False)      # warm-up: code objects, pinned buffers
            for _ in range(a.reps):
                for k, (p, knob) in legs.items():
                    if knob is None:
                        os.environ.pop("VGH_DEVICE_FASTA", None)
                    else:
                        os.environ["VGH_DEVICE_FASTA"] = knob
                    t = time.perf_counter()
                    _, _, hist, st = g.sample_count(ctx, [p], threads=16, require_depth=False)
                    dt = time.perf_counter() - t
                    rates[k].append(st["n_reads"] / dt)
                    stats[k] = (st["n_reads"], st["read_base"], hist.tobytes())
            os.environ.pop("VGH_DEVICE_FASTA", None)
            assert all(v == stats["fasta"] for v in stats.values()), "the legs count differently"
            assert stats["fasta"][:2] == (n_reads, n_reads * L)
            med = {k: statistics.median(v) for k, v in rates.items()}
            twin = rates["fastq_twin"]
            files[name + ("_bgzf" if bgzf else "_plain")] = {
                "reads": n_reads, "read_len": L, "line_width": width, "make_s": round(t_make, 1),
                "bytes": {"fasta": os.path.getsize(fa), "fastq_twin": os.path.getsize(fq)},
                "reads_per_s": {k: float("%.4g" % v) for k, v in med.items()},
                "runs": {k: ["%.4g" % x for x in v] for k, v in rates.items()},
                "fasta_over_today": round(med["fasta"] / med["fasta_today"], 2) if "fasta_today" in med else None,
                "fasta_over_twin": round(med["fasta"] / med["fastq_twin"], 3),
                "twin_spread": ["%.4g" % min(twin), "%.4g" % max(twin)],
                "faster_than_today": bool(med["fasta"] > med["fasta_today"]) if "fasta_today" in med else None,
                "at_least_twin": bool(med["fasta"] >= med["fastq_twin"]),
                "within_twin_spread": bool(med["fasta"] >= min(twin)),
            }
            tmp.cleanup()
            print(name, "bgzf" if bgzf else "plain", json.dumps(files[name + ("_bgzf" if bgzf else "_plain")]["reads_per_s"]), file=sys.stderr, flush=True)
    out = {"tool": "bench_fasta", "reps": a.reps, "level": a.level, "member_text_bytes": 0xff00, "files": files}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        open(a.out, "w").write(line + "\n")
    ctx.close()
    g.close()


if __name__ == "__main__":
    main()
