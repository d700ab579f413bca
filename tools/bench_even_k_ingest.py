#!/usr/bin/env python3
"""FASTQ files -> counters (vgh_sample_count, reads/s) for one k and one build, a container per line: plain, block gzip, ordinary gzip.

The measurement of DESIGN_INGEST_HMM.md 4.17: even k behind the device-side readers against the parent commit's build, where an
even-k sample takes the host reader for the whole file.  One process is one run of one build; `--root` names the tree whose package
and libraries are measured (default: this file's), `--work` a directory both builds share -- the first run writes the graph
(`varigraph-mi construct -k K`) and the read files there, every later one reuses them, so two builds count the same bytes.  The
counters' digest is printed too: it must be the same for every container and for both builds.

  python tools/bench_even_k_ingest.py --k 22 --genome 1000000 --variants 1000 --pairs 2000000 --work /tmp/w22 [--root OTHER_TREE]
"""
import argparse
import gzip
import hashlib
import json
import os
import shutil
import subprocess
import sys
import threading
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--work", required=True)
    ap.add_argument("--k", type=int, required=True)
    ap.add_argument("--genome", type=int, default=1_000_000)
    ap.add_argument("--variants", type=int, default=1000)
    ap.add_argument("--pairs", type=int, default=2_000_000)
    ap.add_argument("--threads", type=int, default=8)
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    sys.path.insert(0, a.root)
    from varigraph_amd import host, synth, vgmi
    os.makedirs(a.work, exist_ok=True)
    graph = os.path.join(a.work, f"graph_k{a.k}.bin")
    prefix = os.path.join(a.work, "s")
    if not os.path.exists(graph) or not os.path.exists(prefix + ".done"):
        ref = synth.make_reference(a.genome)
        variants, gts = synth.make_cohort(ref, a.variants, n_samples=5, ploidy=2, seed=11)
    if not os.path.exists(graph):
        fa, vcf = os.path.join(a.work, "ref.fa"), os.path.join(a.work, "in.vcf")
        synth.write_fasta(fa, "chr1", ref)
        synth.write_vcf(vcf, "chr1", len(ref), variants, gts, 5, 2)
        cli = os.path.join(a.root, "varigraph_amd", "bin", "varigraph-mi")
        r = subprocess.run([cli, "construct", "-r", fa, "-v", vcf, "--save-graph", graph + ".tmp", "-t", "16", "--gpu", "0", "-k", str(a.k)], cwd=a.work,
                           capture_output=True, text=True, env=dict(os.environ, VGH_RANDOM_DEVICE_VALUE="20241022"), timeout=900)
        assert r.returncode == 0, r.stderr[-2000:]
        os.replace(graph + ".tmp", graph)
    plain = [prefix + "_1.fq", prefix + "_2.fq"]
    if not os.path.exists(prefix + ".done"):
        haps = synth.sample_haplotypes(ref, variants, gts, 0, 2)
        synth.write_fastq_pair_device(prefix, haps, a.pairs, 77)

        def pack(p):
            with open(p, "rb") as fi, gzip.open(p + ".gz", "wb", compresslevel=4) as fo:
                shutil.copyfileobj(fi, fo, 1 << 24)
            synth.bgzf_compress_file(p, p + ".bgz.gz", level=4)
        ts = [threading.Thread(target=pack, args=(p,)) for p in plain]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        open(prefix + ".done", "w").write("ok\n")
    files = {"plain": plain, "bgzf": [p + ".bgz.gz" for p in plain], "gzip": [p + ".gz" for p in plain]}
    g = host.Graph(graph)
    ctx = vgmi.Context(0, buffer_mib=128)
    g.upload(ctx)
    n_reads = 2 * a.pairs
    out = {"label": a.label, "k": a.k, "genome": a.genome, "n_reads": n_reads, "threads": a.threads, "host_parse": os.environ.get("VGH_HOST_PARSE", "")}
    g.sample_count(ctx, files["plain"], threads=a.threads, require_depth=False)      # (the streams' buffers are allocated here, not in a timed call)
    digest = None
    for name, paths in files.items():
        t0 = time.perf_counter()
        cov, _, _, st = g.sample_count(ctx, paths, threads=a.threads, require_depth=False)
        dt = time.perf_counter() - t0
        assert st["n_reads"] == n_reads
        d = hashlib.sha1(cov.tobytes()).hexdigest()
        assert digest in (None, d), name
        digest = d
        out[name + "_reads_per_s"] = round(n_reads / dt)
    out["counters_sha1"] = digest
    ctx.close()
    g.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
