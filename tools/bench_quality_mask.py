#!/usr/bin/env python3
"""FASTQ files -> counters (vgh_sample_count_q, reads/s) with and without a minimum base quality, a container per line: plain, block
gzip, ordinary gzip.

The measurement of DESIGN_INGEST_HMM.md 4.20: what fq_pack_mask_kernel costs next to fq_pack_kernel on the same files.  The reads are
those of the committed C1 graph's sample (tests/golden/c1), 2 x 150 bp, written with four quality values drawn 80 / 10 / 7 / 3 %
('F' ':' ',' '#' = Q37, Q25, Q11, Q2: what a binned instrument writes), so --q 20 masks a tenth of the bases.  One untimed plain call
first (the streams' buffers are allocated there) and one per container (the inflate scratch), then `--runs` rounds per container of
two timed windows, option off and option on alternately; a window repeats the call until `--window` seconds have passed (a single
call of 2e6 reads takes 16 to 40 ms: too little to time) and its rate is reads counted over the window's wall time, every call ending
in the read-back of the counters.  masked_bases is checked against the quality bytes of the files in every call.

  python tools/bench_quality_mask.py --work /tmp/qm [--pairs 1000000] [--q 20] [--runs 5] [--window 1.0]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--work", required=True)
    ap.add_argument("--pairs", type=int, default=1_000_000)
    ap.add_argument("--q", type=int, default=20)
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
    low = 0
    for p in plain:        # the model's count: quality bytes below 33 + q
        m = np.fromfile(p, dtype=np.uint8).reshape(a.pairs, -1)
        low += int((m[:, 17 + 150:17 + 300] < 33 + a.q).sum())

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
    out = {"n_reads": n_reads, "threads": a.threads, "q": a.q, "window_s": a.window, "bases_below_q": low,
           "fraction_below_q": low / (n_reads * 150.0), "runs": []}
    for paths in files.values():
        g.sample_count(ctx, paths, threads=a.threads, require_depth=False)
    ref_cov = {}
    for _ in range(a.runs):
        row = {}
        for name, paths in files.items():
            for q in (0, a.q):
                calls, t0 = 0, time.perf_counter()
                while calls == 0 or time.perf_counter() - t0 < a.window:
                    cov, _, _, st = g.sample_count(ctx, paths, threads=a.threads, require_depth=False, min_base_quality=q)
                    calls += 1
                    assert st["n_reads"] == n_reads and st["masked_bases"] == (low if q else 0), (name, q, st["masked_bases"], low)
                dt = time.perf_counter() - t0
                assert np.array_equal(ref_cov.setdefault(q, cov), cov), (name, q)
                row[f"{name}_q{q}_reads_per_s"] = round(calls * n_reads / dt)
                row[f"{name}_q{q}_calls"] = calls
        out["runs"].append(row)
    assert not np.array_equal(ref_cov[0], ref_cov[a.q])
    for key in out["runs"][0]:
        if key.endswith("_reads_per_s"):
            vals = [r[key] for r in out["runs"]]
            out["median_" + key], out["min_" + key], out["max_" + key] = int(np.median(vals)), min(vals), max(vals)
    ctx.close()
    g.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
