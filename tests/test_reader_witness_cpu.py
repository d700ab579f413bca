"""The cases of tests/reader_witness.py are what they claim (no device): the witness table sees every read byte, the case families
cover the residues, lengths and limits they name -- each claim computed from the case data and asserted as a full set --, the host
reader (the restated kseq) returns the model's reads on every case file, and wrong parsers written as variants of the model give other
counters than the true one."""
import itertools
import math

import numpy as np
import pytest

import oracle_lib as o
import reader_witness as W
from varigraph_amd import host

_TABLES = {}


def _table(k):
    if k not in _TABLES:
        _TABLES[k] = o.Table(W.keys(k))
    return _TABLES[k]


def _counts(block, k):
    t = _table(k)
    t.reset()
    if block:
        t.count_block(np.frombuffer(block, dtype=np.uint8), k)
    return t.counts()


def test_the_witness_genome_and_its_tables():
    """all 6 000 circular 27-mers are distinct keys, under the small-graph kernels' 65 536; the k = 11 table holds nearly as many"""
    assert len(W.G) == 6000 and W.keys(W.K).size == 6000 < 65536
    assert 5900 < W.keys(W.K_SHORT).size <= 6000
    lens = W.witness_lengths()
    assert sum(lens) == len(W.G) and min(lens) >= 27 and max(lens) <= 160
    assert b"".join(W.reads_of(W.get("witness_tiles").text, "fastq")) == W.G
    for k in (W.K, W.K_SHORT):
        c = _counts(W.block_of([W.G + W.G[:k - 1]]), k)
        assert c.min() >= 1 and (k == W.K_SHORT or c.max() == 1)


def _read_spans(block):
    """(first, end) of every read of a block"""
    out, a = [], 0
    for e in np.flatnonzero(np.frombuffer(block, dtype=np.uint8) == 10).tolist():
        out.append((a, e))
        a = e + 1
    return out


@pytest.mark.parametrize("name,k", [("witness_tiles", W.K), ("lengths", W.K), ("lengths", W.K_SHORT), ("sweep_fastq_m1", W.K),
                                    ("sweep_fasta_m1", W.K)])
def test_every_read_byte_is_counted(name, k):
    """Every single-base substitution, every single-byte deletion -- separators included, the final newline excepted -- and every
    newline inserted inside a read changes the oracle's counters.  The ones that cannot: a change inside a read shorter than k, and
    the loss of a separator between two reads shorter than k together; the test asserts that the invisible changes are exactly those
    (none for the tiles of 27 bases and more).  Their bases are held by n_bases, which the GPU tests compare as well."""
    block = W.model(W.get(name)).block
    base = _counts(block, k)
    assert base.any()
    spans = _read_spans(block)
    read_of = {}
    for i, (a, e) in enumerate(spans):
        for p in range(a, e + 1):
            read_of[p] = i
    length = [e - a for a, e in spans]
    nxt = dict(zip(b"ACGT", b"CGTA"))
    seen = {"sub": [0, 0], "del": [0, 0], "nl": [0, 0]}

    def check(kind, changed, must_show, what):
        shows = not np.array_equal(_counts(changed, k), base)
        assert shows == must_show, (name, k, kind, what)
        seen[kind][0] += shows
        seen[kind][1] += 1
    for p in range(len(block)):
        i = read_of[p]
        if block[p] != 10:
            check("sub", block[:p] + bytes([nxt[block[p]]]) + block[p + 1:], length[i] >= k, p)
            check("del", block[:p] + block[p + 1:], length[i] >= k or length[i] == 1, p)      # (an empty read: the oracle refuses the block)
            if p > spans[i][0]:
                check("nl", block[:p] + b"\n" + block[p:], length[i] >= k, p)
        elif p + 1 < len(block):
            check("del", block[:p] + block[p + 1:], length[i] + length[i + 1] >= k, p)
    print(name, k, {kind: "%d of %d" % tuple(v) for kind, v in seen.items()})
    if min(length) >= k:
        assert seen["sub"][0] == seen["sub"][1] == sum(length) and seen["del"][0] == seen["del"][1] == len(block) - 1


def test_a_base_doubled_at_a_reads_end_shows_in_n_bases_only():
    """what the counters do not see: the first or last base of a read written twice (the k-mers stay); n_bases differs"""
    block = W.model(W.get("witness_tiles")).block
    a, e = _read_spans(block)[3]
    for p in (a, e - 1):
        twice = block[:p] + block[p:p + 1] + block[p:]
        assert np.array_equal(_counts(twice, W.K), _counts(block, W.K)) and len(twice) - twice.count(b"\n") == len(W.G) + 1


# ---- coverage ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", W.names("sweep"))
def test_sweep_chunk_ends_and_carried_starts(name):
    c = W.get(name)
    R, m = W.record_bytes(c), W.model(c)
    assert R >= 16 and not m.stopped
    assert all(n <= c.cap for n in c.pieces)
    if "_m" in name:
        assert (c.pieces[0] - 1) % R == 0 and len(m.ends) >= R
        assert {e % R for e in m.ends} == set(range(R))                              # chunk ends visit every offset of a record
        assert {(W.TAIL_MAX - t) % 16 for t in m.tails} == set(range(16))            # and the carry's start every residue mod 16
    else:
        assert c.pieces[0] < R and math.gcd(c.pieces[0], R) == 1
        assert {e % R for e in m.ends[:-1]} == set(range(R))
        grow = [len(list(g)) for up, g in itertools.groupby(b > a for a, b in zip(m.tails, m.tails[1:])) if up]
        assert max(grow) >= 2          # a tail that grows over several commits: chunks without a complete record
    whole = W.reads_of(c.text, c.kind)
    assert m.reads == (whole if c.kind == "fastq" else whole[:-1])
    assert W.model(c, None).reads == m.reads and len(W.model(c, None).ends) == 1


def test_lengths_and_mask_cases():
    assert [len(r) for r in W.model(W.get("lengths")).reads] == list(W.LENGTHS)
    assert len(W.names("mask")) == 18
    for name in W.names("mask"):
        c = W.get(name)
        q, where = c.min_quality, name.split("_", 2)[2]
        m = W.model(c)
        want = [W.low_positions(where, n) for n in W.LENGTHS]
        assert [{i for i, b in enumerate(r) if b == ord("N")} for r in m.reads] == want, name
        assert m.masked_bases == sum(map(len, want)) and (where == "none") == (m.masked_bases == 0)
        quals = set(b"".join(c.text.split(b"\n")[3::4]))
        assert quals <= {33 + q - 1, 33 + q} and (where == "every") == (quals == {33 + q - 1})
    assert W.low_positions("63_and_64", 64) == {63} and W.low_positions("63_and_64", 65) == {63, 64}


@pytest.mark.parametrize("name", W.names("subsample"))
def test_subsample_chunks(name):
    """a dropped read is the first, the last and the only record of a chunk, and dropped reads run in a row"""
    c = W.get(name)
    f, seed = c.subsample
    m = W.model(c)
    n_all = len(W.reads_of(c.text, c.kind))
    keep = [W.S.keep(i, seed, f) for i in range(n_all)]
    R = len(c.text) // n_all
    assert len(c.text) % n_all == 0 and all(p % R == 0 for p in c.pieces)
    chunks, a = [], 0
    for e in m.ends:
        chunks.append(keep[a:e // R])
        a = e // R
    if c.kind == "fasta":          # the last record of a chunk is carried: the chunks' records lag by one
        chunks = [keep[max(a - 1, 0):b - 1] for a, b in zip([0] + [e // R for e in m.ends[:-1]], [e // R for e in m.ends])]
    chunks = [x for x in chunks if x]
    assert any(x == [False] for x in chunks) and any(len(x) > 1 and not x[0] for x in chunks) and any(len(x) > 1 and not x[-1] for x in chunks)
    assert W.S.longest_dropped_run(keep) >= 2
    assert m.n_seen == (n_all if c.kind == "fastq" else n_all - 1) and m.n_records == sum(keep[:m.n_seen]) and 0 < m.n_records < m.n_seen


def test_fa_copy_covers_every_class():
    short, long_, groups = (W.model(W.get("fa_copy_" + n)) for n in ("short_lines", "long_lines", "groups_of_four"))
    for m in (short, long_, groups):
        assert len(m.ends) == 1 and not m.stopped and {c[0] for c in m.copies} == {0}
    # (one commit: the chunk starts at the carry's end, a multiple of 16, so offsets in the raw buffer are file offsets)
    text = W.get("fa_copy_short_lines").text
    assert all(text[raw - W.TAIL_MAX:raw - W.TAIL_MAX + n] == short.block[dst:dst + n] for _, _, raw, dst, n in short.copies)
    got = {(raw % 4, dst % 4, n) for _, _, raw, dst, n in short.copies}
    assert got >= set(itertools.product(range(4), range(4), range(1, 21)))
    got = {(raw % 4, dst % 16, n) for _, _, raw, dst, n in long_.copies}
    assert got >= set(itertools.product(range(4), range(16), range(511, 544)))
    assert 0 < _counts(long_.block, W.K).max() < 255          # G over and over: the counters stay below saturation
    masks = {}
    for _, i, _, _, n in groups.copies:
        masks.setdefault(i // 4, [0, 0])
        masks[i // 4][0] |= (n >= W.FA_LONG) << (i % 4)
        masks[i // 4][1] += 1
    assert {m for m, n in masks.values() if n == 4} == set(range(16))      # 0 .. 4 long lines of a step's four, in each position
    c = W.get("fa_copy_short_lines_cut_behind_a_line")
    m = W.model(c)
    assert c.text[m.ends[0] - 1:m.ends[0] + 1] == b"\n>" and m.reads == short.reads and m.tails[0] > 0
    assert all(len(r) >= W.K for r in short.reads + long_.reads + groups.reads)


def test_fa_lines_cuts():
    c = W.get("fa_lines")
    m, t = W.model(c), c.text
    assert not t.endswith(b"\n") and not m.stopped
    reads = W.reads_of(t, "fasta")
    assert m.reads == reads[:-1] and b"".join(reads) == W.genome(0, sum(map(len, reads)))
    ends = m.ends[:-1]
    for head in (b">", b"@"):
        assert any(t[e:e + 1] == head for e in ends)                                         # the record begins the next chunk
        assert any(t[e - 1:e] == head for e in ends)                                         # one byte of its header line ends the chunk
        assert any(t[e - 1:e] == b"\n" and t.rfind(b"\n", 0, e - 1) + 1 == t.rfind(head, 0, e) for e in ends)   # a header line is the chunk's last
    assert any(t[e - 1:e + 1] == b"\n\n" for e in ends)                                      # the cut lies in front of an empty line
    assert any(t[e - 2:e] == b"\n\n" for e in ends)                                          # and behind one
    assert b"\n\n\n" in t


@pytest.mark.parametrize("name", W.names("carry") + W.names("line_cap"))
def test_limits_and_one_past(name):
    c = W.get(name)
    m = W.model(c)
    reads, past = W.reads_of(c.text, c.kind), "one_past" in name
    assert m.stopped == past and all(n <= c.cap for n in c.pieces or [0])
    if c.family == "carry":
        assert c.chunk_kb is None and c.cap_lines == ((512 << 20) + W.TAIL_MAX) // 6
        if c.kind == "fastq":
            assert len(reads[3]) * 2 + len(c.text.split(b"\n")[12]) + 5 == W.TAIL_MAX + 100      # the record's bytes
            assert m.ends[0] - len(W.fastq(reads[:3])) == W.TAIL_MAX + past                      # its first piece
            assert (m.tails[0] == W.TAIL_MAX) == (not past)
        else:
            rec = c.text.index(b">b0") - c.text.index(b">L")
            assert rec == W.TAIL_MAX + past
            assert (m.tails[0] == W.TAIL_MAX) == (not past and "across" in name)
        assert m.reads == (reads[:3] if past else reads if c.kind == "fastq" else reads[:-1])
        assert m.consumed == (c.text.index(b"L") - 1 if past else len(c.text) - len(m.tail))
        assert 80 < _counts(W.block_of(reads), W.K).max() < 255
    else:
        assert len(c.text) == 1 << 20 == c.cap and c.text.count(b"\n") == c.cap_lines + past and c.cap_lines == 349525
        assert (m.n_records, m.consumed) == ((0, 0) if past else (c.cap_lines // 4, len(c.text) - len(m.tail)))
        assert sorted(map(len, set(reads)))[-5:] == [90, 91, 92, 93, 94] and len(reads) + 1 == len(W.reads_of(c.file, "fastq")) == c.cap_lines // 4 + 1
    assert m.tail == (b"" if past else c.text[m.consumed:])


# ---- the host reader and the model check each other ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", W.names())
def test_host_reader_returns_the_models_reads(name, tmp_path):
    c = W.get(name)
    p = tmp_path / ("x.fq" if c.kind == "fastq" else "x.fa")
    p.write_bytes(c.file)
    reads, masked, seen = W.whole(c)
    if c.subsample:
        block, n, rb, mb, nx = host.reads_read_all_s(str(p), c.subsample[0], c.subsample[1], min_base_quality=c.min_quality)
        assert (mb, nx) == (masked, seen)
    elif c.min_quality:
        block, n, rb, mb = host.reads_read_all_q(str(p), c.min_quality)
        assert mb == masked
    else:
        block, n, rb = host.fastx_read_all(str(p))
    assert block.tobytes() == W.block_of(reads) and (n, rb) == (len(reads), sum(map(len, reads)))
    # the model's stream: a front part of those reads, and with the tail's reads all of them unless the device stopped
    m = W.model(c)
    assert m.reads == reads[:len(m.reads)] and (m.n_records, m.n_bases) == (len(m.reads), sum(map(len, m.reads)))
    assert m.consumed + len(m.tail) == len(c.text) or m.stopped
    if not m.stopped and c.file == c.text and not c.subsample:
        rest = [W.Q.mask(r, q, c.min_quality)[0] for r, q in zip(W.reads_of(m.tail, c.kind), m.tail.split(b"\n")[3::4])] if c.min_quality \
            else W.reads_of(m.tail, c.kind) if b"\n" in m.tail or c.kind == "fasta" else []
        assert m.reads + rest == reads


def test_the_witness_graph_loads(tmp_path):
    p = tmp_path / "graph.bin"
    p.write_bytes(W.graph_bin(W.K))
    a = host.load_graph(str(p))
    assert a["k"] == W.K and np.array_equal(a["keys"], W.keys(W.K)) and a["node_off"].tolist() == [0, 40]
    assert a["node_key_index"].tolist() == list(range(40)) and a["chr_names"] == ["chrW"] and a["genome_size"] == len(W.G)


# ---- wrong parsers ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bug,where", [("mask_shifted_by_one", "mask_q20_first"),
                                       ("mask_shifted_by_one", "mask_q20_63_and_64"),
                                       ("line_loses_last_byte_at_dst_3_mod_4", "fa_copy_short_lines"),
                                       ("line_loses_last_byte_at_dst_3_mod_4", "fa_lines"),
                                       ("long_line_from_source_rounded_down_to_4", "fa_copy_long_lines"),
                                       ("long_line_from_source_rounded_down_to_4", "fa_copy_groups_of_four"),
                                       ("subsample_numbers_from_the_chunk", "subsample_0.5_seed_11"),
                                       ("subsample_numbers_from_the_chunk", "subsample_0.5_fasta"),
                                       ("chunk_end_loses_the_tails_first_byte", "sweep_fastq_m1"),
                                       ("chunk_end_loses_the_tails_first_byte", "sweep_fasta_m1")])
def test_a_wrong_parser_gives_other_counters(bug, where):
    assert bug in W.BUGS
    c = W.get(where)
    assert not np.array_equal(_counts(W.model(c, bug=bug).block, W.K), _counts(W.model(c).block, W.K))
