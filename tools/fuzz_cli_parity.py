#!/usr/bin/env python3
"""Drawn end-to-end cases through both CLIs (the unmodified reference, oracle/_ref/varigraph_det, and varigraph-mi) on one GPU box:
genome size, variant mix, cohort size and ploidy, k, construct mode, reads per sample and every genotype option are drawn from a seed;
graph.bin and every VCF must be byte-identical, or both must refuse.  Prints one line per case and the parameters of any difference.
  fuzz_cli_parity.py <first seed> <cases> [--k K] [--genome G] [--max-ploidy N] [--max-vcf-samples N] [--only-wide-ploidy] [--subsample] [--bam-filter] [--bam-regions] [--read-filter]
--max-ploidy N (default 4: every seed draws the case it always drew) adds ploidy 5 .. N to what the cohort's and the sample's ploidy are drawn from.
--max-vcf-samples N (default 7: every seed draws the case it always drew) adds cohorts of 24, 33, 48, 64, 100, 127, 130, 160 and 255 diploid
VCF samples, as far as N allows, to what a diploid cohort's size is drawn from: graphs of 49 to 511 haplotypes, 7 to 64 bytes of haplotype bits
per k-mer (N = 127 draws what it drew before the last three were added; a seed's case depends on N, as it always has).
--only-wide-ploidy runs, of the seeds given, only those whose draw is a polyploid sample (ploidy 3 and more) over a cohort of 49 or more
haplotypes (DESIGN_INGEST_HMM 4.18; with VGH_HMM_WIDE_PLOIDY_DEVICE=1 in the environment the device path of such samples); the others are
passed over before anything is built.  Every seed keeps its case.
--subsample (off by default: every seed draws the case it always drew) gives half of the cases a fraction and a seed for `genotype --subsample`,
drawn from a generator of their own behind the case's; varigraph-mi then reads the case's files with the option and the reference the
filtered files this script writes with the Python model of the rule (tests/subsample_cases.py): the same VCFs, or both refuse.
--bam-filter (off by default, and only for cases --subsample left alone) turns the read files of half of the cases into BAM files with
drawn flags, MAPQ and an rq field, and draws a read filter (DESIGN_INGEST_HMM 4.23): varigraph-mi reads the BAM files with the filter's
options, the reference the twin FASTQ of the records that pass by the Python model (tests/bam_filter_cases.py).
--bam-regions (off by default, and only for cases the two options above left alone) turns the read files of half of the cases into aligned
BAM files over four references with drawn positions and CIGARs, and draws a region list, a BED file or both, with or without
--bam-regions-unplaced (DESIGN_INGEST_HMM 4.24): varigraph-mi reads the BAM files with the options, the reference the twin FASTQ of the
records that pass by the Python model (tests/bam_region_cases.py).
--read-filter (off by default, and only for cases the three options above left alone) gives half of the cases drawn parameters for
`genotype --min-read-length / --max-read-length / --min-read-quality / --max-low-quality` (DESIGN_INGEST_HMM 4.25) and draws the
qualities of the case's reads afresh, read by read, from five profiles, so that every test drops some: varigraph-mi reads the case's
files with the options, the reference the twin files of the reads that pass by the Python model (tests/read_filter_cases.py).
  fuzz_cli_parity.py --check-bam-regions <first seed> <cases>
needs no device: the conversion alone -- drawn records, regions and option text -- through the host decoder (vgh_reads_read_all_r)
against the model's passing records."""
import gzip, os, shutil, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import importlib.util
import numpy as np
spec = importlib.util.spec_from_file_location("tc", os.path.join(ROOT, "tests", "test_gpu_configs.py"))
tc = importlib.util.module_from_spec(spec); spec.loader.exec_module(tc)
from varigraph_amd import synth


def dress(path, rng):
    """A FASTQ file as sequencers and pipelines leave them (round 5): some reads with N, some in lower case, some cut short (ragged
    lengths), then plain / gzip at a drawn level / gzip of several members / block gzip.  Returns the path to put into samples.cfg."""
    import zlib
    lines = open(path, "rb").read().split(b"\n")
    n_rec = len(lines) // 4
    for r in rng.choice(n_rec, size=max(1, n_rec // 40), replace=False):
        seq, qual = bytearray(lines[4 * r + 1]), lines[4 * r + 3]
        what = int(rng.integers(0, 4))
        if what == 0:
            for pos in rng.integers(0, len(seq), size=int(rng.integers(1, 4))): seq[int(pos)] = ord("N")
        elif what == 1:
            seq = bytearray(bytes(seq).lower())
        elif what == 2:
            cut = int(rng.integers(1, len(seq)))
            seq, qual = seq[:cut], qual[:cut]
        else:
            a = int(rng.integers(0, len(seq) - 2))
            seq[a:a + 2] = b"NN"
        lines[4 * r + 1], lines[4 * r + 3] = bytes(seq), qual
    text = b"\n".join(lines)
    form = int(rng.integers(0, 5))
    if form == 0:
        open(path, "wb").write(text)
        return path
    if form == 1 or form == 2:
        level = int(rng.integers(1, 10))
        open(path + ".gz", "wb").write(gzip.compress(text, compresslevel=level))
        os.remove(path)
        return path + ".gz"
    if form == 3:      # several members, cut anywhere
        cuts = sorted(set([0, len(text)] + [int(x) for x in rng.integers(0, len(text), size=int(rng.integers(1, 6)))]))
        with open(path + ".gz", "wb") as f:
            for a, b in zip(cuts[:-1], cuts[1:]): f.write(gzip.compress(text[a:b], compresslevel=6))
        os.remove(path)
        return path + ".gz"
    open(path, "wb").write(text)
    synth.bgzf_compress_file(path, path + ".gz", level=int(rng.integers(1, 10)), block=int(rng.integers(2000, 0xff01)))
    os.remove(path)
    return path + ".gz"


MAX_PLOIDY = 4      # --max-ploidy N: ploidy 5 .. N joins both draws (DESIGN_INGEST_HMM 4.15: the device's HMM for samples of ploidy 5 .. 8)
MAX_VCF_SAMPLES = 7      # --max-vcf-samples N: diploid cohorts of up to N samples (DESIGN_INGEST_HMM 4.16, 4.21: the device's HMM over panels of 48 to 511 haplotypes)
ONLY_WIDE_PLOIDY = False      # --only-wide-ploidy: seeds whose draw is anything else are passed over
BAM_FILTER = False      # --bam-filter: a drawn case may get BAM read files and a read filter (DESIGN_INGEST_HMM 4.23)
SUBSAMPLE = False      # --subsample: a drawn case may get a fraction and a seed (DESIGN_INGEST_HMM 4.22)
FORCE = {}      # --k K / --genome G on the command line: the drawn value replaced (round 6: campaigns of k = 28 over graphs on either side of 65 536 k-mers)


def filtered(path, fraction, sub_seed):
    """the reads of a FASTQ file (plain, gzip of any number of members, block gzip) that the rule keeps, as a plain four-line file"""
    import subsample_cases
    raw = open(path, "rb").read()
    text = gzip.decompress(raw) if raw[:2] == b"\x1f\x8b" else raw
    if not text.endswith(b"\n"): text += b"\n"
    out = path + ".kept.fq"
    open(out, "wb").write(subsample_cases.filtered_fastq_text(text, fraction, sub_seed)[0])
    return out


READ_FILTER = False      # --read-filter: a drawn case may get the read filter by length and read quality (DESIGN_INGEST_HMM 4.25)


def draw_read_filter(qrng):
    """-> (the options, the model's rule): at least one of the four parameters is on"""
    import read_filter_cases as R
    while True:
        min_len, max_len = int(qrng.choice((0, 0, 50, 120))), int(qrng.choice((0, 0, 0, 140, 150)))
        q_text = str(qrng.choice(("0", "0", "7.5", "10", "12.3", "20.0")))
        low = (None, None, (15, 40), (10, 20), (20, 0))[int(qrng.integers(0, 5))]
        if max_len and max_len < min_len: continue
        if min_len or max_len or q_text != "0" or low: break
    opts = []
    if min_len: opts += ["--min-read-length", str(min_len)]
    if max_len: opts += ["--max-read-length", str(max_len)]
    if q_text != "0": opts += ["--min-read-quality", q_text]
    if low: opts += ["--max-low-quality", f"{low[0]}:{low[1]}"]
    whole, _, frac = q_text.partition(".")
    return opts, R.Rule(min_len, max_len, int(whole) * 10 + int(frac or 0), *(low or (0, 0)))


def redraw_qualities(path, qrng):
    """the quality lines of a plain four-line FASTQ file drawn afresh, a profile per read (read_filter_cases.drawn_quality)"""
    import read_filter_cases as R
    lines = open(path, "rb").read().split(b"\n")
    for i in range(3, len(lines), 4):
        lines[i] = R._ph(R.drawn_quality(qrng, len(lines[i]), int(qrng.choice((0, 0, 0, 0, 1, 2, 3, 4)))))
    open(path, "wb").write(b"\n".join(lines))


def passing(path, rule):
    """the reads of a FASTQ file (plain, gzip of any number of members, block gzip) that pass the rule, as a plain four-line file"""
    import read_filter_cases as R
    raw = open(path, "rb").read()
    text = gzip.decompress(raw) if raw[:2] == b"\x1f\x8b" else raw
    if not text.endswith(b"\n"): text += b"\n"
    out = path + ".pass.fq"
    open(out, "wb").write(R.filtered_fastq_text(text, rule)[0])
    return out


BAM_FILTERS = ((["--bam-exclude-flags", "0xF00"], dict(exclude=0xF00)), (["--bam-exclude-flags", "0x400"], dict(exclude=0x400)),
               (["--bam-min-mapq", "20"], dict(min_mapq=20)), (["--bam-min-tag", "rq:0.99"], dict(tag=b"rq", min_value=0.99)),
               (["--bam-exclude-flags", "0xD00", "--bam-require-flags", "0x1", "--bam-min-mapq", "5", "--bam-min-tag", "rq:0.95"],
                dict(exclude=0xD00, require=0x1, min_mapq=5, tag=b"rq", min_value=0.95)))


def as_bam(path, brng, filt):
    """a read file of the case as a BAM with drawn flags, MAPQ and rq -> (the BAM, the twin FASTQ of the records that pass `filt`)"""
    import bam_filter_cases as F, bam_py, quality_mask_cases
    raw = open(path, "rb").read()
    text = gzip.decompress(raw) if raw[:2] == b"\x1f\x8b" else raw
    if not text.endswith(b"\n"): text += b"\n"
    recs = []
    for name, seq, qual in quality_mask_cases.records_of(text):
        flag = (1 if brng.random() < 0.7 else 0) | (0x10 if brng.random() < 0.5 else 0)
        for bit, p in ((0x100, 0.03), (0x200, 0.05), (0x400, 0.12), (0x800, 0.03)):
            if brng.random() < p: flag |= bit
        rq = 1.0 - 0.1 * float(brng.random()) ** 3      # (0.9, 1]: 46 % at or above 0.99, 79 % at or above 0.95
        recs.append(bam_py.Rec(name.split()[0], seq.upper(), flag=flag, mapq=int(brng.choice((0, 3, 20, 60, 255))), qual=bytes(min(max(c - 33, 0), 93) for c in qual),
                               aux=F.aux(b"NM", "C", 2) + F.aux(b"RG", "Z", b"g1") + F.aux(b"rq", "f", rq)))
    bam_py.write_bam(path + ".bam", recs, level=int(brng.integers(1, 7)), block=int(brng.integers(2000, 0xff01)))
    passing, _, _, at = F.apply(recs, F.Filter(**filt))
    assert at is None
    return path + ".bam", bam_py.twin_fastq(path + ".twin.fq", passing)


BAM_REGIONS = False      # --bam-regions: a drawn case may get aligned BAM read files and regions (DESIGN_INGEST_HMM 4.24)


def draw_regions(rrng, work):
    """-> (the options, the intervals as the model takes them, unplaced): one whole reference or none, 1 to 40 intervals on the others,
    as --bam-regions items, as lines of a BED file (with lines the header lacks), or both"""
    import bam_region_cases as R
    names = [n.decode() for n, _ in R.REFS]
    regions, items, lines = [], [], ["# drawn", "chrUn\t5\t50"]
    whole = int(rrng.integers(-1, len(names)))
    if whole >= 0:
        regions.append((whole, 0, R.WHOLE)); items.append(names[whole])
    for _ in range(int(rrng.integers(1, 41))):
        ref, beg = int(rrng.integers(0, len(names))), int(rrng.integers(0, 2500))
        end = beg + int(rrng.integers(1, 200))
        regions.append((ref, beg, end))
        if rrng.random() < 0.5: items.append(f"{names[ref]}:{beg + 1}-{end}")
        else: lines.append(f"{names[ref]}\t{beg}\t{end}")
    if rrng.random() < 0.2:      # NAME:BEG, to the end
        ref, beg = int(rrng.integers(0, len(names))), int(rrng.integers(1500, 2500))
        regions.append((ref, beg, R.WHOLE)); items.append(f"{names[ref]}:{beg + 1}")
    opts = []
    if items: opts += ["--bam-regions", ",".join(items)]
    if len(lines) > 2:
        bed = os.path.join(work, "regions.bed")
        open(bed, "w").write("\n".join(lines + ["chrEBV\t1\t2"]) + "\n")
        opts += ["--bam-regions-file", bed]
    unplaced = bool(rrng.random() < 0.5)
    return opts + (["--bam-regions-unplaced"] if unplaced else []), regions, unplaced


def as_region_bam(path, rrng, regions, unplaced):
    """a read file of the case as an aligned BAM with drawn references, positions and CIGARs -> (the BAM, the twin FASTQ of the records
    that pass the regions, those records)"""
    import bam_filter_cases as F, bam_py, bam_region_cases as R, quality_mask_cases
    raw = open(path, "rb").read()
    text = gzip.decompress(raw) if raw[:2] == b"\x1f\x8b" else raw
    if not text.endswith(b"\n"): text += b"\n"
    recs = []
    for name, seq, qual in quality_mask_cases.records_of(text):
        q = bytes(min(max(c - 33, 0), 93) for c in qual)
        if rrng.random() < 0.05:
            recs.append(bam_py.Rec(name.split()[0], seq.upper(), flag=4, ref=-1, pos=-1, mapq=0, qual=q))
            continue
        flag = (0x10 if rrng.random() < 0.5 else 0) | (4 if rrng.random() < 0.05 else 0) | (0x100 if rrng.random() < 0.03 else 0)
        cigar = [(int(rrng.integers(1, 60)), R.OPS[int(rrng.integers(0, 9))] if rrng.random() < 0.97 else int(rrng.integers(9, 16)))
                 for _ in range(int(rrng.integers(0, 6)))]
        recs.append(bam_py.Rec(name.split()[0], seq.upper(), flag=flag, ref=int(rrng.integers(0, len(R.REFS))), pos=int(rrng.integers(-1, 2700)),
                               mapq=int(rrng.choice((0, 20, 60))), cigar=cigar, qual=q, aux=F.aux(b"NM", "C", 2)))
    R.write_bam(path + ".bam", recs)
    passing, _, _, at = R.apply(recs, F.Filter(), regions, unplaced)
    assert at is None
    return path + ".bam", bam_py.twin_fastq(path + ".twin.fq", passing), passing


def check_bam_regions(seed):
    """the conversion without a device: a drawn FASTQ file -> as_region_bam -> the host decoder with the drawn options == the passing records"""
    import bam_py
    from varigraph_amd import host
    rrng = np.random.default_rng([int(seed), 0xBA4E])
    work = tempfile.mkdtemp(prefix="fuzz_regions_")
    try:
        fq = os.path.join(work, "r.fq")
        with open(fq, "wb") as f:
            for i in range(int(rrng.integers(50, 600))):
                n = int(rrng.integers(30, 160))
                f.write(b"@r%d\n" % i + synth._ACGT[rrng.integers(0, 4, size=n)].tobytes() + b"\n+\n" + bytes(rrng.integers(35, 74, size=n, dtype=np.uint8)) + b"\n")
        opts, regions, unplaced = draw_regions(rrng, work)
        bam, twin, passing = as_region_bam(fq, rrng, regions, unplaced)
        arg = lambda o: opts[opts.index(o) + 1] if o in opts else None
        block, n, rb = host.reads_read_all_r(bam, arg("--bam-regions"), arg("--bam-regions-file"), unplaced)[:3]
        want = bam_py.reads_block(passing)
        twin_n = open(twin, "rb").read().count(b"\n") // 4
        ok = block.tobytes() == want[0] and (n, rb) == want[1:] and twin_n == n
        return ("identical (%d of the file's reads pass)" % n if ok else "CONVERSION DIFFERS"), f"seed {seed}: {' '.join(opts)}"
    finally:
        shutil.rmtree(work, ignore_errors=True)


def case(seed):
    rng = np.random.default_rng(seed)
    pick = lambda xs: xs[int(rng.integers(0, len(xs)))]
    genome = int(pick([40_000, 90_000, 200_000, 400_000, 1_500_000, 1_500_000]))      # (the last: more than 65 536 k-mers with dense variants -- the context table at any k)
    more_ploidy = list(range(5, MAX_PLOIDY + 1))
    vploidy = pick([2, 2, 2, 3, 4] + more_ploidy)
    more_samples = [n for n in (24, 33, 48, 64, 100, 127, 130, 160, 255) if n <= MAX_VCF_SAMPLES]
    n_samples = pick([1, 2, 3, 5, 7] + more_samples) if vploidy <= 2 else pick([1, 2, 3])
    k = pick([27, 27, 27, 21, 25, 22, 28, 15, 11, 19, 23, 20, 24, 26])
    k = FORCE.get("k", k)
    genome = FORCE.get("genome", genome)
    if k < 19 and genome > 400_000: genome = 400_000      # (the reference takes minutes over 1.5 Mb of 11- and 15-mers)
    copts = pick([[], [], ["--fast"], ["--use-unique-kmers"]])
    n_var = max(5, genome // pick([300, 600, 1500]))
    indel, sv = pick([0.0, 0.1, 0.3]), pick([0.0, 0.01, 0.05])
    sploidy = pick([2, 2, 2, 3, 4] + more_ploidy)
    gopts = ["-g", pick(["het", "het", "hom"]), "-m", pick(["rec", "fre"]), "--sample-ploidy", str(sploidy), "-n", str(pick([1, 2, 4, 7, 15, 15, 40]))]
    if rng.random() < 0.3: gopts += ["--sv"]
    if rng.random() < 0.4: gopts += ["--use-depth"]
    if rng.random() < 0.3: gopts += ["--min-support", str(pick([5, 30, 80]))]
    if rng.random() < 0.5: gopts += ["--granularity", str(pick([0.003, 0.02, 0.1]))]
    n_reads_samples = pick([1, 1, 2, 3])
    pairs = int(pick([3_000, 15_000, 40_000]))
    desc = f"seed {seed}: genome {genome}, {n_var} variants (indel {indel}, sv {sv}), cohort {n_samples} x ploidy {vploidy}, k {k}, construct {copts}, {n_reads_samples} samples x {pairs} pairs, genotype {' '.join(gopts)}"
    if ONLY_WIDE_PLOIDY and not (sploidy >= 3 and n_samples * vploidy + 1 >= 49): return "passed over", desc
    work = tempfile.mkdtemp(prefix="fuzz_")
    try:
        ref = synth._ACGT[rng.integers(0, 4, size=genome)]
        variants, gts = synth.make_cohort(ref, n_var, n_samples=n_samples, ploidy=vploidy, seed=int(seed) + 1, indel_frac=indel, sv_frac=sv)
        fa, vcf = os.path.join(work, "ref.fa"), os.path.join(work, "in.vcf")
        synth.write_fasta(fa, "chr1", ref); synth.write_vcf(vcf, "chr1", len(ref), variants, gts, n_samples, vploidy)
        graphs, rcs = {}, {}
        for name, exe, more in (("native", tc.CLI, ["--gpu", "0"]), ("cpu", tc.REF, [])):
            graphs[name] = os.path.join(work, f"g_{name}.bin")
            try:
                r = subprocess.run([exe, "construct", "-r", fa, "-v", vcf, "--save-graph", graphs[name], "-t", "6", "-k", str(k), "--vcf-ploidy", str(vploidy)] + copts + more,
                                   cwd=work, capture_output=True, text=True, env=tc.ENV, timeout=150)
            except subprocess.TimeoutExpired:
                return f"TIMEOUT of {name} (construct)", desc
            rcs[name] = r.returncode
        if (rcs["native"] == 0) != (rcs["cpu"] == 0): return "CONSTRUCT STATUS DIFFERS " + str(rcs), desc
        if rcs["cpu"] != 0: return "both refuse construct", desc
        if open(graphs["native"], "rb").read() != open(graphs["cpu"], "rb").read(): return "GRAPH DIFFERS", desc
        cfg, cfg_kept, sub = "", "", None
        if SUBSAMPLE:      # a generator of its own: the case's draws stay what they were
            srng = np.random.default_rng([int(seed), 0x5AB5])
            if srng.random() < 0.5:
                sub = ([0.5, 0.25, 0.9, 0.05, 0.999][int(srng.integers(0, 5))], int(srng.integers(0, 2 ** 63)) * 2 + int(srng.integers(0, 2)))
                desc += f", --subsample {sub[0]} --subsample-seed {sub[1]}"
        bamf = None
        if BAM_FILTER and sub is None:      # a generator of its own, as above
            brng = np.random.default_rng([int(seed), 0xBA3F])
            if brng.random() < 0.5:
                bamf = BAM_FILTERS[int(brng.integers(0, len(BAM_FILTERS)))]
                desc += ", BAM read files, " + " ".join(bamf[0])
        regf = None
        if BAM_REGIONS and sub is None and bamf is None:      # a generator of its own, as above
            rrng = np.random.default_rng([int(seed), 0xBA4E])
            if rrng.random() < 0.5:
                regf = draw_regions(rrng, work)
                desc += ", aligned BAM read files, " + " ".join(regf[0])
        rff = None
        if READ_FILTER and sub is None and bamf is None and regf is None:      # a generator of its own, as above
            qrng = np.random.default_rng([int(seed), 0x4EAD])
            if qrng.random() < 0.5:
                rff = draw_read_filter(qrng)
                desc += ", drawn qualities, " + " ".join(rff[0])
        for i in range(n_reads_samples):
            who = int(rng.integers(0, n_samples))
            haps = synth.sample_haplotypes(ref, variants, gts, who, vploidy)
            fq = tc._write_fastq(os.path.join(work, f"s{i}"), haps, pairs, seed=int(seed) * 10 + i)
            if rff:
                for f in fq: redraw_qualities(f, qrng)
            fq = [dress(f, rng) for f in fq]
            cfg += f"ind{i} " + " ".join(fq) + "\n"
            if rff: cfg_kept += f"ind{i} " + " ".join(passing(f, rff[1]) for f in fq) + "\n"
            if sub: cfg_kept += f"ind{i} " + " ".join(filtered(f, *sub) for f in fq) + "\n"
            if bamf:
                pairs_ = [as_bam(f, brng, bamf[1]) for f in fq]
                cfg = cfg[:cfg.rindex(f"ind{i} ")] + f"ind{i} " + " ".join(b for b, _ in pairs_) + "\n"
                cfg_kept += f"ind{i} " + " ".join(t for _, t in pairs_) + "\n"
            if regf:
                pairs_ = [as_region_bam(f, rrng, regf[1], regf[2])[:2] for f in fq]
                cfg = cfg[:cfg.rindex(f"ind{i} ")] + f"ind{i} " + " ".join(b for b, _ in pairs_) + "\n"
                cfg_kept += f"ind{i} " + " ".join(t for _, t in pairs_) + "\n"
        outs, codes = {}, {}
        for name, exe, more in (("native", tc.CLI, ["--gpu", "0"]), ("cpu", tc.REF, [])):
            d = os.path.join(work, name); os.makedirs(d)
            open(os.path.join(d, "samples.cfg"), "w").write(cfg_kept if (sub or bamf or regf or rff) and name == "cpu" else cfg)
            if rff and name == "native": more = more + rff[0]
            if bamf and name == "native": more = more + bamf[0]
            if regf and name == "native": more = more + regf[0]
            if sub and name == "native": more = more + ["--subsample", repr(sub[0]), "--subsample-seed", str(sub[1])]
            try:
                r = subprocess.run([exe, "genotype", "--load-graph", graphs["cpu"], "-s", "samples.cfg", "-t", "6"] + gopts + more, cwd=d, capture_output=True, text=True, env=tc.ENV, timeout=150)
            except subprocess.TimeoutExpired:
                return f"TIMEOUT of {name}", desc
            codes[name] = r.returncode
            if r.returncode != 0:
                codes[name + "_stderr"] = r.stderr.strip().split("\n")[-1][:300]
            if r.returncode == 0:
                outs[name] = [gzip.open(os.path.join(d, f"ind{i}.varigraph.vcf.gz"), "rb").read() for i in range(n_reads_samples)]
        if (codes["native"] == 0) != (codes["cpu"] == 0): return "GENOTYPE STATUS DIFFERS " + str(codes), desc
        if codes["cpu"] != 0: return "both refuse genotype", desc
        for i in range(n_reads_samples):
            if outs["native"][i] != outs["cpu"][i]:
                a, b = outs["native"][i].split(b"\n"), outs["cpu"][i].split(b"\n")
                first = next((j for j, (x, y) in enumerate(zip(a, b)) if x != y), -1)
                return f"VCF {i} DIFFERS at line {first}: {a[first][:160] if first >= 0 else ''} | {b[first][:160] if first >= 0 else ''}", desc
        return f"identical ({sum(o.count(10) for o in outs['cpu'])} VCF lines)", desc
    finally:
        shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    if sys.argv[1] == "--check-bam-regions":
        first, n = int(sys.argv[2]), int(sys.argv[3])
        bad = 0
        for s in range(first, first + n):
            verdict, desc = check_bam_regions(s)
            bad += "DIFFERS" in verdict
            print(("!! " if "DIFFERS" in verdict else "ok ") + verdict + " -- " + desc[:200], flush=True)
        print(f"{n} conversions, {bad} differences")
        sys.exit(1 if bad else 0)
    first, n = int(sys.argv[1]), int(sys.argv[2])
    for i, a in enumerate(sys.argv):
        if a in ("--k", "--genome"): FORCE[a[2:]] = int(sys.argv[i + 1])
        if a == "--max-ploidy": MAX_PLOIDY = int(sys.argv[i + 1])
        if a == "--max-vcf-samples": MAX_VCF_SAMPLES = int(sys.argv[i + 1])
        if a == "--only-wide-ploidy": ONLY_WIDE_PLOIDY = True
        if a == "--subsample": SUBSAMPLE = True
        if a == "--bam-filter": BAM_FILTER = True
        if a == "--bam-regions": BAM_REGIONS = True
        if a == "--read-filter": READ_FILTER = True
    bad = passed_over = 0
    for s in range(first, first + n):
        t0 = time.time()
        verdict, desc = case(s)
        if verdict == "passed over":
            passed_over += 1
            continue
        flag = verdict.isupper() or "DIFFERS" in verdict or "TIMEOUT of native" in verdict      # (the reference's own pool loses a wake-up now and then: skipped, not a difference)
        bad += flag
        print(("!! " if flag else "ok ") + verdict + f" [{time.time() - t0:.1f} s] -- " + desc, flush=True)
    print(f"{n - passed_over} cases, {bad} differences" + (f" ({passed_over} seeds passed over)" if passed_over else ""))
    sys.exit(1 if bad else 0)
