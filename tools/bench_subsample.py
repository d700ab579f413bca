#!/usr/bin/env python3
"""FASTQ files -> counters (vgh_sample_count_s, file reads/s) with and without subsampling, a container per line: plain, block gzip,
ordinary gzip.

The measurement of DESIGN_INGEST_HMM.md 4.22: what the *_sub kernels (a rule per record, a kept count, a copy that skips) cost or save
next to the default path on the same files.  The files are those of tools/bench_quality_mask.py: the reads of the committed C1 graph's
sample (tests/golden/c1), 2 x 150 bp, four quality values.  One untimed call per container first (the streams' buffers and the
inflate scratch are allocated there), then `--runs` rounds per container of two timed windows, option off and option on alternately;
a window repeats the call until `--window` seconds have passed (a single call of 2e6 reads takes tens of milliseconds: too little to
time).  The rate is the FILE's reads -- kept or not: the whole text is moved, inflated and parsed either way -- over the window's
wall time, every call ending in the read-back of the counters.  reads_seen / reads_kept are checked against the rule's model in
every call.

  python tools/bench_subsample.py --work /tmp/ss [--pairs 1000000] [--fraction 0.5] [--seed 11] [--runs 5] [--window 1.0]
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


def kept_of_first(n, fraction, seed):
    """how many of reads 0 .. n - 1 the rule keeps (the model of tests/subsample_cases.py)"""
    with np.errstate(over="ignore"):
        x = (np.arange(n, dtype=np.uint64) + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(seed)
        x ^= x >> np.uint64(30)
        x *= np.uint64(0xBF58476D1CE4E5B9)
        x ^= x >> np.uint64(27)
        x *= np.uint64(0x94D049BB133111EB)
        x ^= x >> np.uint64(31)
    return int((x < np.uint64(int(fraction * 2 ** 64))).sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--work", required=True)
    ap.add_argument("--pairs", type=int, default=1_000_000)
    ap.add_argument("--fraction", type=float, default=0.5)
    ap.add_argument("--seed", type=int, default=11)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--threads", type=int, default=8)
    ap.add_argument("--window", type=float, default=1.0, help="seconds of repeated calls per timed window")
    a = ap.parse_args()
    sys.path.insert(0, a.root)
    from varigraph_amd import host, synth, vgmi
    os.makedirs(a.work, exist_ok=True)
    gdir = os.path.join(a.root, "tests", "golden", "c1")
    meta = json.load(open(os.path.join(gdir, "meta.json")))
    ref = synth.make_reference(meta["ref_len"], seed=meta["ref_seed"])
    variants, gts = synth.make_cohort(ref, meta["n_var"], n_samples=meta["n_samples"], ploidy=meta["ploidy"], seed=meta["cohort_seed"])
    haps = synth.sample_haplotypes(ref, variants, gts, 0, meta["ploidy"])
    n_reads = 2 * a.pairs
    block = vgmi.synth_reads_host(1000, 0, n_reads, 150, haps)
    plain = synth.write_fastq_pair_fast(os.path.join(a.work, "s"), block, n_reads, 150, qual="binned")
    kept = 2 * kept_of_first(a.pairs, a.fraction, a.seed)      # the two files of the pair keep the same numbers

    def pack(p):
        with open(p, "rb") as fi, gzip.open(p + ".gz", "wb", compresslevel=4) as fo:
            shutil.copyfileobj(fi, fo, 1 << 24)
        synth.bgzf_compress_file(p, p + ".bgz.gz", level=4)
    ts = [threading.Thread(target=pack, args=(p,)) for p in plain]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    files = {"plain": plain, "bgzf": [p + ".bgz.gz" for p in plain], "gzip": [p + ".gz" for p in plain]}
    g = host.Graph(os.path.join(gdir, "graph.bin.gz"))
    ctx = vgmi.Context(0, buffer_mib=128)
    g.upload(ctx)
    out = {"n_reads": n_reads, "threads": a.threads, "fraction": a.fraction, "seed": a.seed, "window_s": a.window, "reads_kept": kept,
           "runs": []}
    for paths in files.values():
        g.sample_count(ctx, paths, threads=a.threads, require_depth=False)
    ref_cov = {}
    for _ in range(a.runs):
        row = {}
        for name, paths in files.items():
            for on in (False, True):
                calls, t0 = 0, time.perf_counter()
                while calls == 0 or time.perf_counter() - t0 < a.window:
                    cov, _, _, st = g.sample_count(ctx, paths, threads=a.threads, require_depth=False,
                                                   subsample=(a.fraction, a.seed) if on else None)
                    calls += 1
                    if on:
                        assert (st["reads_seen"], st["reads_kept"], st["n_reads"]) == (n_reads, kept, kept), (name, st)
                    else:
                        assert st["n_reads"] == n_reads, (name, st)
                dt = time.perf_counter() - t0
                assert np.array_equal(ref_cov.setdefault(on, cov), cov), (name, on)
                tag = "sub" if on else "off"
                row[f"{name}_{tag}_file_reads_per_s"] = round(calls * n_reads / dt)
                row[f"{name}_{tag}_calls"] = calls
        out["runs"].append(row)
    assert not np.array_equal(ref_cov[False], ref_cov[True])
    for key in out["runs"][0]:
        if key.endswith("_reads_per_s"):
            vals = [r[key] for r in out["runs"]]
            out["median_" + key], out["min_" + key], out["max_" + key] = int(np.median(vals)), min(vals), max(vals)
    ctx.close()
    g.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
