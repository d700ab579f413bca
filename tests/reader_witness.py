"""Read files for the device FASTQ / FASTA parsers (csrc/vgmi_fastq.hip, csrc/vgmi_fasta.hip) in which every read byte is counted, and
the plain-Python model of what the parsers must make of them.  No device involved: test_reader_witness_cpu.py proves the cases are what
they claim, test_gpu_reader_witness.py runs them.

The witness: a seeded random genome G, read as a circle, and the table of ALL its canonical k-mers (k = 27: under 65 536 keys, so the
small-graph kernels count them; k = 11 for the reads shorter than 27 bases).  Reads are consecutive, non-overlapping stretches of G in
genome order, so a garbled base removes key k-mers, a lost separator between two records makes k-mers that are keys, and a dropped or
doubled read moves counters down or up.  The parsers' read block never leaves the device; the counters of this table are the view of it.

The model (model()) walks the commits as the C ABI receives them and parses the text line by line: FASTQ = line 2 of every four-line
group; FASTA = the sequence lines of a record joined, the last record of the data left as the tail; --min-base-quality by
quality_mask_cases.mask, --subsample by the keep rule of subsample_cases.  The documented refusals are part of it: a record longer
than the 1 MiB carry and a chunk of more than cap_lines lines stop the device at a record's first byte.

A case carries its text, its commit sizes (None: whole staging buffers) and the VGMI_FASTQ_CHUNK_KB it needs (None: the default
geometry, 512 MiB of text per chunk behind 16 MiB staging buffers)."""
import itertools
import struct

import numpy as np

import oracle_lib as o
import quality_mask_cases as Q
import subsample_cases as S

K, K_SHORT = 27, 11
TAIL_MAX = 1 << 20                   # csrc/vgmi_api_fastq.cpp: the carry between chunks
STAGING_MIB = 16                     # the GPU tests' Context(buffer_mib=16)
FA_LONG = 512                        # csrc/vgmi_fasta.hip: a line of this many bytes or more is copied by its whole wavefront
LENGTHS = (1, 2, 3, 26, 27, 28, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257)
_NONE = np.uint64(0xFFFFFFFFFFFFFFFF)

G = np.frombuffer(b"ACGT", dtype=np.uint8)[np.random.default_rng(5).integers(0, 4, size=6000)].tobytes()


def genome(pos, n):
    """n bases of the circle from pos on"""
    pos %= len(G)
    return (G * ((pos + n) // len(G) + 1))[pos:pos + n]


def keys(k):
    """every canonical k-mer of the circle, once"""
    ks = np.unique(o.sketch(G + G[:k - 1], k))
    return ks[ks != _NONE]


def tiles(lengths, pos=0):
    out = []
    for n in lengths:
        out.append(genome(pos, n))
        pos += n
    return out


def witness_lengths():
    """tile lengths 27 .. 160 that use up G exactly"""
    rng, out, left = np.random.default_rng(6), [], len(G)
    while left:
        n = int(rng.integers(27, 161))
        if left - n < 27:
            n = left if left <= 160 else left - 27
        out.append(n)
        left -= n
    return out


def chunk_cap(chunk_kb):
    """bytes a commit takes at most: the staging buffer"""
    return chunk_kb << 10 if chunk_kb else STAGING_MIB << 20


def cap_lines(chunk_kb):
    """vgmi_fastq_open: (text per chunk + carry) / 6"""
    return ((chunk_kb << 10 if chunk_kb else 512 << 20) + TAIL_MAX) // 6


def commit_sizes(n_text, pieces, cap):
    """what Context._text_stream commits: a size per call, the last one from there on, never more than the buffer or the text left"""
    out, pos, i = [], 0, 0
    while True:
        want = cap if pieces is None else min(pieces[min(i, len(pieces) - 1)], cap)
        n = min(want, n_text - pos)
        out.append(n)
        pos += n
        i += 1
        if pos >= n_text:
            return out


# ---- text builders ---------------------------------------------------------------------------------------------------------------------
def qual_line(i, n):
    """n quality bytes in '#' .. 'J', varied; some lines start with '@', '+' or '>'"""
    return ((np.arange(n) * 7 + i * 13) % 40 + 35).astype(np.uint8).tobytes()


def fastq(reads, quals=None, names=None):
    out = []
    for i, r in enumerate(reads):
        out.append(b"@" + (names[i] if names else b"r%d" % i) + b"\n" + r + b"\n+\n" + (quals[i] if quals else qual_line(i, len(r))) + b"\n")
    return b"".join(out)


def wrap(seq, width):
    return [seq[a:a + width] for a in range(0, len(seq), width)] if width else [seq]


def fasta(reads, width=None, names=None):
    out = []
    for i, r in enumerate(reads):
        out.append(b">" + (names[i] if names else b"r%d" % i) + b"\n" + b"".join(ln + b"\n" for ln in wrap(r, width)))
    return b"".join(out)


def reads_of(text, kind):
    """Every read of a whole file, its last record included: FASTQ line 2 of each four-line group, FASTA the sequence lines of a
    record joined (a line starting with '>' or '@' is a header line, empty lines are passed over)."""
    lines = text.split(b"\n")
    if kind == "fastq":
        return [lines[i + 1] for i in range(0, len(lines) - 3, 4)]
    out = []
    for ln in lines:
        if ln[:1] in (b">", b"@"):
            out.append([])
        elif ln:
            out[-1].append(ln)
    return [b"".join(x) for x in out]


def block_of(reads):
    return b"".join(r + b"\n" for r in reads)


# ---- the model ---------------------------------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, name, family, kind, text, pieces=None, chunk_kb=64, tables=(K,), min_quality=0, subsample=None, file=None,
                 again_in_one_commit=True):
        self.name, self.family, self.kind, self.text, self.pieces, self.chunk_kb = name, family, kind, text, pieces, chunk_kb
        self.tables, self.min_quality, self.subsample = tables, min_quality, subsample
        self.file = text if file is None else file          # what the product path and the host reader read (the text and its rest)
        self.again_in_one_commit = again_in_one_commit
        self.cap, self.cap_lines = chunk_cap(chunk_kb), cap_lines(chunk_kb)

    @property
    def env(self):
        return {"VGMI_FASTQ_CHUNK_KB": str(self.chunk_kb)} if self.chunk_kb else {}


class Result:
    """what the device must report for a stream, the read block its counters must be the oracle's on, and what the model saw on the way:
    tails = the carried bytes after every commit, copies = (commit, line number in the chunk, offset in the raw buffer, offset in the
    chunk's block, length) of every FASTA sequence line copied"""

    def __init__(self):
        self.reads, self.n_records, self.n_bases, self.consumed, self.stopped = [], 0, 0, 0, False
        self.masked_bases, self.n_seen, self.tails, self.copies, self.ends = 0, 0, [], [], []
        self.tail = b""

    @property
    def block(self):
        return block_of(self.reads)

    def report(self, case):
        out = (self.n_records, self.n_bases, self.consumed, self.stopped, self.tail)
        if case.min_quality:
            out += (self.masked_bases,)
        if case.subsample:
            out += (self.n_seen,)
        return out


BUGS = ("mask_shifted_by_one", "line_loses_last_byte_at_dst_3_mod_4", "long_line_from_source_rounded_down_to_4",
        "subsample_numbers_from_the_chunk", "chunk_end_loses_the_tails_first_byte")


def _keep(st, case, r, bug):
    if not case.subsample:
        return True
    f, seed = case.subsample
    return S.keep((0 if bug == "subsample_numbers_from_the_chunk" else st.n_seen) + r, seed, f)


def _take(st, read):
    st.reads.append(read)
    st.n_records += 1
    st.n_bases += len(read)


def _fastq_chunk(st, text, end, case, bug, region):
    lines = region.split(b"\n")[:-1]
    good, off = 0, 0
    for r in range(len(lines) // 4):
        h, s, p, q = lines[4 * r:4 * r + 4]
        if not (h[:1] == b"@" and len(s) >= 1 and s[:1] not in (b"@", b"+", b">") and p[:1] == b"+" and len(q) == len(s)):
            st.stopped = True
            break
        if _keep(st, case, r, bug):
            if case.min_quality:
                s, n = Q.mask(s, q[1:] + q[:1] if bug == "mask_shifted_by_one" else q, case.min_quality)
                st.masked_bases += n
            _take(st, s)
        good += 1
        off += len(h) + len(s) + len(p) + len(q) + 4
    st.n_seen += good
    st.consumed += off


def _fasta_chunk(st, text, end, case, bug, region, commit):
    raw0 = TAIL_MAX - (st.tails[-1] if st.tails else 0)       # where the region starts in the raw buffer
    if region[:1] not in (b">", b"@"):
        st.stopped = True
        return
    parts = region.split(b"\n")
    lines = parts[:-1] + ([parts[-1]] if parts[-1] else [])
    recs, pos = [], 0              # [position, [(line number, position, bytes)], has a '+' line]
    for i, ln in enumerate(lines):
        c = ln[:1]
        if c in (b">", b"@"):
            recs.append([pos, [], False])
        elif c == b"+":
            recs[-1][2] = True
        elif c:
            recs[-1][1].append((i, pos, ln))
        pos += len(ln) + 1
    H = len(recs)
    first_bad = min([r for r in range(H) if recs[r][2]] +
                    [r for r in range(H - 1) if not recs[r][1] or recs[r + 1][0] - recs[r][0] > TAIL_MAX] + [H])
    good = min(first_bad, H - 1)
    st.stopped = first_bad < H
    dst = 0
    for r in range(good):
        if not _keep(st, case, r, bug):
            continue
        read = b""
        for i, p, ln in recs[r][1]:
            st.copies.append((commit, i, raw0 + p, dst, len(ln)))
            if bug == "line_loses_last_byte_at_dst_3_mod_4" and dst % 4 == 3:
                ln = ln[:-1] + b"N"
            if bug == "long_line_from_source_rounded_down_to_4" and len(ln) >= FA_LONG:
                a = st.consumed + p - (raw0 + p) % 4
                ln = text[a:a + len(ln)]
            read += ln
            dst += len(ln)
        dst += 1
        _take(st, read)
    st.n_seen += good
    st.consumed += recs[good][0]


def model(case, pieces="as cut", bug=None):
    """the stream of case.text committed in case.pieces (or in `pieces`) -> Result"""
    st, end, text = Result(), 0, case.text
    for commit, n in enumerate(commit_sizes(len(text), case.pieces if pieces == "as cut" else pieces, case.cap)):
        end += n
        st.ends.append(end)
        region = text[st.consumed:end]
        if bug == "chunk_end_loses_the_tails_first_byte" and st.tails and st.tails[-1]:
            region = b"N" + region[1:]
        if st.stopped or not region:
            st.tails.append(0)
            continue
        if b"\r" in region or b"\0" in region or region.count(b"\n") > case.cap_lines:
            st.stopped = True          # nothing of this chunk is taken
        elif case.kind == "fastq":
            _fastq_chunk(st, text, end, case, bug, region)
        else:
            _fasta_chunk(st, text, end, case, bug, region, commit)
        if not st.stopped and end - st.consumed > TAIL_MAX:
            st.stopped = True          # a record longer than the carry
        st.tails.append(0 if st.stopped else end - st.consumed)
    st.tail = b"" if st.stopped else text[st.consumed:]
    return st


def whole(case):
    """(reads, masked bases, reads numbered) of the whole of case.file with the case's options: what the device and the host reader that
    takes over from it must have counted between them"""
    reads = reads_of(case.file, case.kind)
    quals = case.file.split(b"\n")[3::4] if case.kind == "fastq" else [None] * len(reads)
    out, masked = [], 0
    for i, (r, q) in enumerate(zip(reads, quals)):
        if case.subsample and not S.keep(i, case.subsample[1], case.subsample[0]):
            continue
        if case.min_quality:
            r, n = Q.mask(r, q, case.min_quality)
            masked += n
        out.append(r)
    return out, masked, len(reads)


# ---- the witness graph as a graph.bin (layout: tests/graphbin_py.py) -------------------------------------------------------------------
def graph_bin(k):
    """A graph.bin whose k-mer records are keys(k): one chromosome, a reference node and one variant node that lists the first keys, one
    diploid sample.  What Graph.sample_count needs to count a read file against the witness table."""
    ks = keys(k)

    def s(b):
        return struct.pack("<I", len(b)) + b

    out = [struct.pack("<QII", len(G), k, 2), s(b"##fileformat=VCFv4.2\n")]
    out.append(struct.pack("<I", 1) + s(b"chrW") + struct.pack("<II", len(G), 0))                 # chromosome lengths, no VCF sites
    out.append(struct.pack("<H", 3) + b"".join(struct.pack("<H", i) + s(n) for i, n in enumerate((b"reference", b"w_1", b"w_2"))))
    out.append(struct.pack("<I", 1) + s(b"chrW") + struct.pack("<I", 2))
    out.append(struct.pack("<II", 1, 1) + s(G[:100]) + struct.pack("<IH", 1, 0) + struct.pack("<I", 0))
    out.append(struct.pack("<II", 101, 2) + s(G[100:101]) + s(b"N") + struct.pack("<IHHH", 3, 0, 0, 1) + struct.pack("<I", 40) + ks[:40].tobytes())
    out.append(struct.pack("<Q", 0))
    rec = np.zeros(ks.size, dtype=np.dtype([("key", "<u8"), ("c", "u1"), ("f", "u1"), ("bl", "<u8"), ("bits", "i1")]))
    rec["key"], rec["f"], rec["bl"], rec["bits"] = ks, 1, 1, 1
    out.append(rec.tobytes())
    return b"".join(out)


# ---- case families -----------------------------------------------------------------------------------------------------------------------
def _sweep():
    out = []
    for kind, n_tile, n_rec in (("fastq", 40, 92), ("fasta", 70, 80)):
        reads = tiles([n_tile] * n_rec)
        names = [b"s%03d" % i for i in range(n_rec)]
        text = fastq(reads, names=names) if kind == "fastq" else fasta(reads, 60, names)
        R = len(text) // n_rec
        # pieces of m * R + 1 bytes, R of them and more: chunk ends visit every offset of a record (m = 1: G has the bases for it)
        out.append(Case("sweep_%s_m1" % kind, "sweep", kind, text, [R + 1]))
        for p in (37, 11):         # shorter than a record, coprime to R: chunks without a complete record, a tail that grows
            out.append(Case("sweep_%s_pieces_of_%d" % (kind, p), "sweep", kind, text, [p], again_in_one_commit=False))
    return out


def record_bytes(case):
    """the one byte size of a sweep case's records"""
    n = len(reads_of(case.text, case.kind))
    assert len(case.text) % n == 0
    return len(case.text) // n


def _lengths():
    w = tiles(witness_lengths())
    return [Case("lengths", "lengths", "fastq", fastq(tiles(LENGTHS)), [100], tables=(K, K_SHORT)),
            Case("witness_tiles", "lengths", "fastq", fastq(w), [1000], tables=(K, K_SHORT))]


MASK_WHERE = ("first", "last", "first_and_last", "63_and_64", "every", "none")


def low_positions(where, n):
    return {"first": {0}, "last": {n - 1}, "first_and_last": {0, n - 1}, "63_and_64": {p for p in (63, 64) if p < n},
            "every": set(range(n)), "none": set()}[where]


def _mask():
    reads, out = tiles(LENGTHS), []
    for q in (1, 20, 93):
        for where in MASK_WHERE:       # quality bytes at bound - 1 (masked) and at bound (kept)
            quals = [bytes(33 + q - (1 if j in low_positions(where, len(r)) else 0) for j in range(len(r))) for r in reads]
            out.append(Case("mask_q%d_%s" % (q, where), "mask", "fastq", fastq(reads, quals), [100], tables=(K, K_SHORT), min_quality=q))
    return out


SUB_PATTERN = (1, 2, 1, 3, 1, 4, 2, 1, 5, 1)       # records per commit, in turn


def _subsample():
    n_rec = 200
    reads = tiles([30] * n_rec)
    names = [b"u%03d" % i for i in range(n_rec)]
    quals = [bytes(33 + (19 if (i + j) % 11 == 0 else 20 + (i + j) % 20) for j in range(30)) for i in range(n_rec)]
    fq, fa = fastq(reads, quals, names), fasta(reads, 20, names)

    def pieces(text):
        R = len(text) // n_rec
        return [R * n for n, _ in zip(itertools.cycle(SUB_PATTERN), range(n_rec))]
    out = []
    for f in (0.5, 0.02):
        for seed in S.SEEDS:
            out.append(Case("subsample_%g_seed_%d" % (f, seed), "subsample", "fastq", fq, pieces(fq), subsample=(f, seed)))
    out.append(Case("subsample_0.5_with_mask", "subsample", "fastq", fq, pieces(fq), subsample=(0.5, 11), min_quality=20))
    out.append(Case("subsample_0.5_fasta", "subsample", "fasta", fa, pieces(fa), subsample=(0.5, 11)))
    return out


def _header(n):
    """a header line of n bytes, newline included (n >= 2)"""
    return b">" + b"h" * (n - 2) + b"\n"


def _fa_copy_short():
    """sequence lines of 1 .. 20 bytes at every (source offset mod 4, destination offset mod 4): header lengths steer the source, the
    lines in front steer the destination; every record is a stretch of G of 27 bases or more"""
    need = {(s, d, n) for s in range(4) for d in range(4) for n in range(1, 21)}
    text, g = [b">filler\n" + genome(0, 40) + b"\n"], 40
    F, B = len(text[0]), 41

    def wanted(s, d):
        return sum((s % 4, d % 4, n) in need for n in range(1, 21))
    while need:
        h = max(range(2, 6), key=lambda h: wanted(F + h, B))
        text.append(_header(h))
        F += h
        size = 0
        while size < 27 or (size < 100 and wanted(F, B)):
            cands = [n for n in range(1, 21) if (F % 4, B % 4, n) in need] or list(range(1, 21))
            n = max(cands, key=lambda n: (wanted(F + n + 1, B + n), n))
            need.discard((F % 4, B % 4, n))
            text.append(genome(g, n) + b"\n")
            g, F, B, size = g + n, F + n + 1, B + n, size + n
        B += 1
    text.append(b">end\n" + genome(g, 30) + b"\n")
    return b"".join(text)


def _fa_copy_long():
    """lines of 511 .. 543 bytes at every (source offset mod 4, destination offset mod 16): a record is a filler line that steers the
    destination and the long line behind it, together one stretch of G"""
    text, g = [b">filler\n" + genome(0, 40) + b"\n"], 40
    F, B = len(text[0]), 41
    for s, d, n in itertools.product(range(4), range(16), range(511, 544)):
        f = (d - B) % 16
        lead = f + 1 if f else 0
        h = 2 + (s - F - lead - 2) % 4
        text.append(_header(h) + (genome(g, f) + b"\n" if f else b"") + genome(g + f, n) + b"\n")
        g, F, B = g + f + n, F + h + lead + n + 1, B + f + n + 1
    text.append(b">end\n" + genome(g, 30) + b"\n")
    return b"".join(text)


def _fa_copy_groups():
    """the four lines a wavefront takes in one step with 0 .. 4 long ones, in each position: empty lines put the header line at line
    4j + 3, the record's four sequence lines are lines 4j + 4 .. 4j + 7"""
    text, g, n_lines = [b">filler\n" + genome(0, 40) + b"\n"], 40, 2
    for m in range(16):
        pad = (3 - n_lines) % 4
        text.append(b"\n" * pad + b">g%02d\n" % m)
        n_lines += pad + 1
        for p in range(4):
            n = FA_LONG + 5 * m + p if m >> p & 1 else 28 + p
            text.append(genome(g, n) + b"\n")
            g += n
        n_lines += 4
    text.append(b">end\n" + genome(g, 30) + b"\n")
    return b"".join(text)


def _fa_copy():
    short, long_, groups = _fa_copy_short(), _fa_copy_long(), _fa_copy_groups()
    last = short.rindex(b">end\n")
    return [Case("fa_copy_short_lines", "fa_copy", "fasta", short, None),
            # cut behind the newline of the last line in front of the last record's header, and again behind that record's own: the
            # carried tail's copy ends on the last byte of the committed data
            Case("fa_copy_short_lines_cut_behind_a_line", "fa_copy", "fasta", short, [last, len(short) - last], again_in_one_commit=False),
            Case("fa_copy_long_lines", "fa_copy", "fasta", long_, None, chunk_kb=2048),
            Case("fa_copy_groups_of_four", "fa_copy", "fasta", groups, None)]


def _fa_lines():
    """empty lines and '@'-headed records on both sides of a chunk end, a header line as the chunk's last line, an unterminated last line"""
    reads = tiles([50 + i % 7 for i in range(60)])
    text, cuts = b"", set()
    for i, r in enumerate(reads):
        at = len(text)
        head = (b"@" if i % 2 else b">") + b"f%02d" % i + (b" +x >y @z" if i % 3 == 0 else b"")
        body = head + b"\n"
        for j, ln in enumerate(wrap(r, 20)):
            body += ln + b"\n" + (b"\n" if (i + j) % 3 == 0 else b"")
        body += b"\n\n" if i % 4 == 0 else b""
        if 2 <= i < len(reads) - 1:
            gap = body.find(b"\n\n")
            where = {0: at, 1: at + 1, 2: at + len(head) + 1, 3: at + len(head), 4: at + gap + 1 if gap >= 0 else at, 5: at + gap + 2 if gap >= 0 else at}
            cuts.add(where[i // 2 % 6])
        text += body
    text = text.rstrip(b"\n")          # the last line is unterminated
    cuts = sorted(c for c in cuts if 0 < c < len(text))
    pieces = [b - a for a, b in zip([0] + cuts, cuts + [len(text)])]
    return [Case("fa_lines", "fa_lines", "fasta", text, pieces)]


def _carry():
    """records at the carry's limit and one past it (default geometry): the long read is G repeated"""
    front, back = tiles([60, 61, 62]), tiles([63, 64, 65], 183)
    out = []
    # FASTQ: a record of 1 MiB + 100 bytes: '@L\n' + seq + '\n+\n' + qual + '\n'
    n = (TAIL_MAX + 100 - 7) // 2
    rec = b"@L\n" + genome(183 + 192, n) + b"\n+\n" + b"I" * n + b"\n"
    rec = rec[:1] + b"L" * (TAIL_MAX + 100 - len(rec)) + rec[1:]
    a, b = fastq(front), fastq(back, names=[b"b%d" % i for i in range(3)])
    text = a + rec + b
    out.append(Case("carry_fastq_tail_equals_the_carry", "carry", "fastq", text, [len(a) + TAIL_MAX, len(text)], chunk_kb=None))
    out.append(Case("carry_fastq_tail_one_past_the_carry", "carry", "fastq", text, [len(a) + TAIL_MAX + 1, len(text)], chunk_kb=None,
                    again_in_one_commit=False))
    # FASTA: records of exactly the carry's bytes and of one more, wrapped at 60
    a, b = fasta(front, 60), fasta(back, 60, names=[b"b%d" % i for i in range(3)])
    for extra in (0, 1):
        body = TAIL_MAX + extra - 3                 # '>L\n' + the lines
        n = body - (body + 60) // 61                # bases: every line of 60 has a newline, and so has the rest
        rec = b">L\n" + b"".join(ln + b"\n" for ln in wrap(genome(183 + 192, n), 60))
        if len(rec) != TAIL_MAX + extra:            # (the rest came out empty: one base less, one byte more of name)
            rec = b">L" + b"L" * (TAIL_MAX + extra - len(rec)) + rec[2:]
        text = a + rec + b
        tag = "one_past" if extra else "equals"
        out.append(Case("carry_fasta_across_commits_%s_the_carry" % tag, "carry", "fasta", text, [len(a) + len(rec), len(text)], chunk_kb=None,
                        again_in_one_commit=False))
        out.append(Case("carry_fasta_in_one_commit_%s_the_carry" % tag, "carry", "fasta", text, None, chunk_kb=None, again_in_one_commit=False))
    return out


def _line_cap():
    """one commit of exactly 1 MiB (VGMI_FASTQ_CHUNK_KB=1024) with cap_lines newlines, and with one more: one-base records padded by
    name length, witness records among them; the text ends inside a record, the file completes it"""
    cap, n_rec = cap_lines(1024), cap_lines(1024) // 4
    wit = dict(zip((0, 1, n_rec // 2, n_rec - 2, n_rec - 1), tiles([90, 91, 92, 93, 94])))
    out = []
    for extra, name in ((0, "line_cap_at_the_limit"), (1, "line_cap_one_past_the_limit")):
        n_nl = cap + extra
        part = {1: b"@last\n" + genome(460, 40), 2: b"@last\n" + genome(460, 40) + b"\n+"}[n_nl - 4 * n_rec]
        rest = {1: b"\n+\n" + b"I" * 40 + b"\n", 2: b"\n" + b"I" * 40 + b"\n"}[n_nl - 4 * n_rec]
        reads = [wit.get(i, b"ACGT"[i % 4:i % 4 + 1]) for i in range(n_rec)]
        spare = (1 << 20) - len(part) - sum(2 * len(r) + 6 for r in reads)
        names = [b"n" * (spare // n_rec + (1 if i < spare % n_rec else 0)) for i in range(n_rec)]
        text = fastq(reads, [b"I" * len(r) for r in reads], names) + part
        out.append(Case(name, "line_cap", "fastq", text, None, chunk_kb=1024, file=text + rest, again_in_one_commit=False))
    return out


_CASES = None


def cases():
    global _CASES
    if _CASES is None:
        _CASES = {c.name: c for c in _sweep() + _lengths() + _mask() + _subsample() + _fa_copy() + _fa_lines() + _carry() + _line_cap()}
    return _CASES


def names(family=None):
    return [n for n, c in cases().items() if family is None or c.family == family]


def get(name):
    return cases()[name]
