#!/usr/bin/env python3
"""FASTQ files -> counters (vgh_sample_count_l, file reads/s and file bases/s) with and without the read filter by length and read
quality, a file set per line: the short-read pair of tools/bench_quality_mask.py (plain, block gzip, ordinary gzip) and a long-read
FASTQ of drawn lengths.

The measurement of DESIGN_INGEST_HMM.md 4.25: what fq_records_rf / fq_read_quality / fq_finish_rf (a wavefront per record over its
quality line, in front of the scan) cost or save next to the default path on the same files.
  short   the reads of the committed C1 graph's sample (tests/golden/c1), 2 x 150 bp, four quality values
  long    reads drawn from the same haplotypes, lengths log-uniform in [--long-min, --long-max] (200 .. 100 000), --long-mb MB of
          bases, qualities of an ONT-like profile: a per-read mean drawn in Q5 .. Q25, per-base values around it
One untimed call per file set first (the streams' buffers and the inflate scratch are allocated there), then `--runs` rounds per set
of two timed windows, option off and option on alternately; a window repeats the call until `--window` seconds have passed.  The
rate is the FILE's reads (and bases) -- kept or not: the whole text is moved, inflated and parsed either way -- over the window's wall
time, every call ending in the read-back of the counters.  The five stats are checked against a numpy model of the rule in every call.

  python tools/bench_read_filter.py --work /tmp/rf [--pairs 1000000] [--long-mb 300] [--runs 5] [--window 1.0]
        [--min-read-length 100] [--max-read-length 0] [--min-read-quality 10.0] [--max-low-quality 15:40]
"""
import argparse
import gzip
import json
import os
import shutil
import sys
import threading
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_read_filter_table import table  # noqa: E402  (the rule's error table, by exact decimal arithmetic)


def model_stats(path, rule, step=200_000):
    """(evaluated, short, long, low fraction, low mean, bases) of a four-line FASTQ file under the rule, in numpy: a running sum of E
    over the quality bytes of `step` records at a time"""
    e10 = np.array(table(), dtype=np.uint64)
    e_of = e10[10 * np.clip(np.arange(256) - 33, 0, 93)]
    data = np.frombuffer(open(path, "rb").read(), dtype=np.uint8)
    nl = np.flatnonzero(data == 10)
    n = len(nl) // 4
    q0, q1 = nl[2:4 * n:4] + 1, nl[3:4 * n:4]
    length = (nl[1:4 * n:4] - nl[0:4 * n:4] - 1).astype(np.uint64)
    assert np.array_equal(q1 - q0, length.astype(np.int64))
    low_byte = 33 + rule["lowq_below"] if rule["lowq_below"] else 0
    cls = np.zeros(n, dtype=np.uint8)
    for a in range(0, n, step):
        b = min(n, a + step)
        seg = data[q0[a]:q1[b - 1]]
        cs_e = np.concatenate(([0], np.cumsum(e_of[seg], dtype=np.uint64)))
        cs_l = np.concatenate(([0], np.cumsum(seg < low_byte, dtype=np.uint64)))
        s, e = q0[a:b] - q0[a], q1[a:b] - q0[a]
        sum_e, n_low, ln = cs_e[e] - cs_e[s], cs_l[e] - cs_l[s], length[a:b]
        c = np.zeros(b - a, dtype=np.uint8)
        if rule["min_mean_q"]:
            c[sum_e > e10[rule["min_mean_q"]] * ln] = 4
        if rule["lowq_below"]:
            c[n_low * np.uint64(100) > np.uint64(rule["lowq_max_pct"]) * ln] = 3
        if rule["max_len"]:
            c[ln > rule["max_len"]] = 2
        c[ln < rule["min_len"]] = 1
        cls[a:b] = c
    return (n,) + tuple(int((cls == k).sum()) for k in (1, 2, 3, 4)) + (int(length.sum()),)


def write_long_reads(path, haps, total_bases, lo, hi, seed):
    """a four-line FASTQ of reads with log-uniform lengths in [lo, hi] until total_bases are written"""
    rng = np.random.default_rng(seed)
    n_reads = 0
    with open(path, "wb") as f:
        left = total_bases
        while left > 0:
            ln = int(np.exp(rng.uniform(np.log(lo), np.log(hi))))
            h = haps[int(rng.integers(0, len(haps)))]
            ln = min(ln, len(h) - 1)
            s0 = int(rng.integers(0, len(h) - ln))
            mean = rng.uniform(5, 25)
            ql = np.clip(np.rint(rng.normal(mean, 5, size=ln)), 1, 50).astype(np.uint8) + 33
            f.write(b"@long%d\n" % n_reads + h[s0:s0 + ln].tobytes().upper() + b"\n+\n" + ql.tobytes() + b"\n")
            n_reads += 1
            left -= ln
    return n_reads


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--work", required=True)
    ap.add_argument("--pairs", type=int, default=1_000_000)
    ap.add_argument("--long-mb", type=int, default=300)
    ap.add_argument("--long-min", type=int, default=200)
    ap.add_argument("--long-max", type=int, default=100_000)
    ap.add_argument("--min-read-length", type=int, default=100)
    ap.add_argument("--max-read-length", type=int, default=0)
    ap.add_argument("--min-read-quality", default="10.0")
    ap.add_argument("--max-low-quality", default="15:40")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--threads", type=int, default=8)
    ap.add_argument("--window", type=float, default=1.0, help="seconds of repeated calls per timed window")
    a = ap.parse_args()
    sys.path.insert(0, a.root)
    from varigraph_amd import host, synth, vgmi
    os.makedirs(a.work, exist_ok=True)
    lq, pct = (int(x) for x in a.max_low_quality.split(":")) if a.max_low_quality else (0, 0)
    rule = dict(min_len=a.min_read_length, max_len=a.max_read_length, min_mean_q=host.parse_quality_tenths(a.min_read_quality), lowq_below=lq,
                lowq_max_pct=pct)
    gdir = os.path.join(a.root, "tests", "golden", "c1")
    meta = json.load(open(os.path.join(gdir, "meta.json")))
    ref = synth.make_reference(meta["ref_len"], seed=meta["ref_seed"])
    variants, gts = synth.make_cohort(ref, meta["n_var"], n_samples=meta["n_samples"], ploidy=meta["ploidy"], seed=meta["cohort_seed"])
    haps = synth.sample_haplotypes(ref, variants, gts, 0, meta["ploidy"])
    files, want = {}, {}
    if a.pairs:
        n_reads = 2 * a.pairs
        block = vgmi.synth_reads_host(1000, 0, n_reads, 150, haps)
        plain = synth.write_fastq_pair_fast(os.path.join(a.work, "s"), block, n_reads, 150, qual="binned")

        def pack(p):
            with open(p, "rb") as fi, gzip.open(p + ".gz", "wb", compresslevel=4) as fo:
                shutil.copyfileobj(fi, fo, 1 << 24)
            synth.bgzf_compress_file(p, p + ".bgz.gz", level=4)
        ts = [threading.Thread(target=pack, args=(p,)) for p in plain]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        files.update({"plain": plain, "bgzf": [p + ".bgz.gz" for p in plain], "gzip": [p + ".gz" for p in plain]})
        per_file = [model_stats(p, rule) for p in plain]
        want["plain"] = want["bgzf"] = want["gzip"] = tuple(sum(v) for v in zip(*per_file))
    if a.long_mb:
        lp = os.path.join(a.work, "long.fq")
        write_long_reads(lp, haps, a.long_mb * 1_000_000, a.long_min, a.long_max, 77)
        files["long_plain"] = [lp]
        want["long_plain"] = model_stats(lp, rule)
    g = host.Graph(os.path.join(gdir, "graph.bin.gz"))
    ctx = vgmi.Context(0, buffer_mib=128)
    g.upload(ctx)
    out = {"threads": a.threads, "rule": rule, "window_s": a.window, "runs": [],
           "files": {k: {"reads": v[0], "bases": v[5], "short": v[1], "long": v[2], "low_fraction": v[3], "low_mean": v[4]} for k, v in want.items()}}
    for paths in files.values():
        g.sample_count(ctx, paths, threads=a.threads, require_depth=False)
    ref_cov = {}
    for _ in range(a.runs):
        row = {}
        for name, paths in files.items():
            n_reads, n_bases = want[name][0], want[name][5]
            for on in (False, True):
                calls, t0 = 0, time.perf_counter()
                while calls == 0 or time.perf_counter() - t0 < a.window:
                    cov, _, _, st = g.sample_count(ctx, paths, threads=a.threads, require_depth=False, read_filter=rule if on else None)
                    calls += 1
                    if on:
                        assert st["read_filter_stats"] == want[name][:5], (name, st["read_filter_stats"], want[name])
                        assert st["n_reads"] == n_reads - sum(want[name][1:5]), (name, st)
                    else:
                        assert (st["n_reads"], st["read_base"]) == (n_reads, n_bases), (name, st)
                dt = time.perf_counter() - t0
                key = (name.startswith("long"), on)
                assert np.array_equal(ref_cov.setdefault(key, cov), cov), (name, on)
                tag = "rf" if on else "off"
                row[f"{name}_{tag}_file_reads_per_s"] = round(calls * n_reads / dt)
                row[f"{name}_{tag}_file_mbases_per_s"] = round(calls * n_bases / dt / 1e6)
                row[f"{name}_{tag}_calls"] = calls
        out["runs"].append(row)
    for key in out["runs"][0]:
        if key.endswith("_per_s"):
            vals = [r[key] for r in out["runs"]]
            out["median_" + key], out["min_" + key], out["max_" + key] = int(np.median(vals)), min(vals), max(vals)
    ctx.close()
    g.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
