"""DEFLATE streams no compressor writes (tests/deflate_builder.py), as a named case list: against zlib here -- the builder's text for
every conformant case, what zlib hands back in front of its error for every other -- and through the host decoder
(csrc/host/fast_inflate.cpp under the sanitizer driver tests/native/inflate_check.cpp).  tests/test_gpu_deflate_shapes.py gives
the same list to the two device decoders.

A case: name, body (DEFLATE bytes), text (what zlib makes of it, up to its error), ok (zlib reaches the stream's end), fastq (the
text is whole four-line FASTQ records), gzip / bgzf (which wrappers it is run in), fields (gzip header with FEXTRA .. FHCRC).

Two things RFC 1951 does not allow and the list therefore holds on the refused side: a dynamic header of HCLEN = 4 gives lengths
to the code-length symbols 16, 17, 18 and 0 only, so every literal/length code length is 0 and there is no end-of-block code (the
fewest that can work is five: case hclen_5); distance symbols 30 / 31 and literal/length symbols 286 / 287 cannot be named by a
dynamic header at all (HDIST <= 30, HLIT <= 286): hdist_31 / hdist_32 / hlit_287 / hlit_288 are those."""
import copy
import os
import subprocess
import zlib

import numpy as np
import pytest

import deflate_builder as db
from deflate_builder import DSym, Dynamic, Fixed, Raw, Stored, Sym

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "varigraph_amd", "csrc", "host")
SEG = 48 << 10           # compressed bytes per guessed block start of the gzip decoder (kGzSeg's default)


def _hap():
    from conftest import get_cohort
    return get_cohort("cohort_snp").haplotypes()[1].tobytes()


def _acgt(n, seed):
    h = _hap()
    s = int(np.random.default_rng(seed).integers(0, len(h) - n))
    return h[s:s + n].upper().replace(b"N", b"A")


def zlib_prefix(body):
    """(what zlib's raw inflate hands back, whether it reached the stream's end); small streams a byte at a time, so that the text
    in front of an error is kept"""
    d, out = zlib.decompressobj(-15), bytearray()
    bulk = max(0, len(body) - 4096) if len(body) < 100_000 else len(body)
    try:
        for i in [0] if bulk else []:
            out += d.decompress(body[:bulk])
        for i in range(bulk, len(body)):
            if d.eof:
                break
            out += d.decompress(body[i:i + 1])
    except zlib.error:
        return bytes(out), False
    return bytes(out), d.eof


def _record(blocks_x, name=b"r0", tail=()):
    """one FASTQ record whose sequence line AND quality line are the text of blocks_x (self-contained: no match reaches in front of
    it), the lines around them in fixed blocks of their own"""
    return ([Fixed(list(b"@" + name + b"\n"))] + copy.deepcopy(blocks_x) + [Fixed(list(b"\n+\n"))] + copy.deepcopy(blocks_x) + [Fixed(list(b"\n"))]
            + list(tail))


def _tokens_text(blocks):
    out = bytearray()
    for b in blocks:
        if isinstance(b, Stored):
            out += b.data
        else:
            out += db.expand(b.tokens, bytes(out))
    return bytes(out)


def _big_fastq(sizes, seed):
    """records of long reads, every line between the structure bytes free to hold planted matches: (text, free mask)"""
    text, free = bytearray(), bytearray()
    for i, n in enumerate(sizes):
        for part, f in ((b"@r%d\n" % i, 0), (_acgt(n, seed + 2 * i), 1), (b"\n+\n", 0), (_acgt(n, seed + 2 * i + 1), 1), (b"\n", 0)):
            text += part
            free += bytes([f]) * len(part)
    return text, free


def _plant(text, free, wants, start):
    """wants: (length, distance[, as 284 + 31]) in the order given, each at the first position at or behind the cursor where the bytes it
    writes and the bytes it reads are free; the text is rewritten to hold the match.  {position: match}"""
    planted, cur = {}, start
    for w in wants:
        length, d = w[0], w[1]
        p = max(cur, d + 8)
        while not (all(free[p:p + length]) and len(free[p:p + length]) == length and all(free[p - d:p - d + min(length, d)])):
            p += 1
            assert p + length < len(text), w
        for i in range(length):
            text[p + i] = text[p - d + i]
        planted[p] = w
        cur = p + length + 3
    return planted


def _regions(text, planted, cuts, kinds):
    """text as blocks: region i = text[cuts[i]:cuts[i + 1]] coded as kinds[i] ('stored', 'fixed', 'dynamic')"""
    blocks = []
    for (a, b), kind in zip(zip(cuts, cuts[1:]), kinds):
        if kind == "stored":
            blocks.append(Stored(text[a:b]))
        else:
            tok = db.tokenize(text[:b], planted={p: m for p, m in planted.items() if a <= p < b}, history=a)
            blocks.append(Fixed(tok) if kind == "fixed" else Dynamic(tok))
    return blocks


SIZES = (8200, 8200, 8200, 7900)      # byte 32768 lies in the second record's quality line


def _case_distances():
    text, free = _big_fastq(SIZES, 100)
    near = [(17, 8960), (258, 3540)]          # from the dynamic block into the stored block and into the fixed block in front of it
    wants = [(l, d) for d in (1, 2, 3, 4, 63, 64, 65, 1280, 1281, 2560, 2561) for l in (3, 16, 17, 258)]
    wants += [(258, d, True) for d in (1, 2, 3, 4, 63, 64, 65, 1280, 1281, 2560, 2561)]
    planted = _plant(text, free, near + wants, 9010)
    assert 9010 in planted and max(planted) < 32700
    # a match at distance 32 768 whose source is the text's very first byte ("@r0" into a quality line)
    assert all(free[32768:32771])
    text[32768:32771] = text[0:3]
    planted[32768] = (3, 32768)
    far = [(l, d) for d in (24577, 32767, 32768) for l in (3, 16, 17, 258)] + [(258, d, True) for d in (24577, 32767, 32768)]
    planted.update(_plant(text, free, far, 32900))
    return bytes(text), _regions(text, planted, [0, 5000, 9000, len(text)], ["stored", "fixed", "dynamic"])


def _case_all_symbols(kind):
    text, free = _big_fastq(SIZES, 200)
    lens = [v for s in range(29) for v in {db.LEN_BASE[s], db.LEN_BASE[s] + (1 << db.LEN_EXTRA[s]) - 1}]
    dists = [v for s in range(30) for v in (db.DIST_BASE[s], db.DIST_BASE[s] + (1 << db.DIST_EXTRA[s]) - 1)]
    lens = sorted(set(lens) | {258})
    wants = [(lens[i % len(lens)], dists[i % len(dists)]) for i in range(max(len(lens), len(dists)) + 7)]
    wants.sort(key=lambda w: w[1])
    planted = _plant(text, free, wants, 33000)
    end = max(planted) + 300
    assert {db._LEN_SYM[w[0]][0] for w in wants} == set(range(257, 286)) and {db.dist_sym(w[1])[0] for w in wants} == set(range(30))
    return bytes(text), _regions(text, planted, [0, 33000, end, len(text)], ["dynamic", kind, "dynamic"])


LONG = list(range(1, 15)) + [15, 15]      # a complete code of lengths 1 .. 14, 15, 15


def _case_long_codes():
    lit_syms = list(b"ACGTNacgt") + [256, 257, 258, 259, 265, 266, 285]
    len_vals = [3, 4, 5, 11, 13, 258]
    dist_syms = [0, 1, 2, 3, 4, 7, 10, 11, 12, 15, 18, 19, 20, 21, 22, 23]
    blocks = [Dynamic(list(_acgt(4200, 7)))]
    for r in range(16):
        ll, dl = [0] * 286, [0] * 30
        for i in range(16):
            ll[lit_syms[(i + r) % 16]] = LONG[i]
            dl[dist_syms[(i + 5 * r) % 16]] = LONG[i]
        tok = []
        for i in range(16):
            tok += list(b"ACGTNacgt"[i % 9:i % 9 + 1]) * (1 + (i + r) % 4)
            tok.append((len_vals[(i + r) % 6], db.DIST_BASE[dist_syms[i]] + (i * 37 + r) % (1 << db.DIST_EXTRA[dist_syms[i]])))
        # (literals under this block's short codes keep the text within eight times the DEFLATE bytes)
        short = [s for s in lit_syms[:9] if 0 < ll[s] <= 9]
        tok += [short[i % len(short)] for i in range(150)]
        blocks.append(Dynamic(tok, lit_lens=ll, dist_lens=dl))
    return blocks


def _case_dense():
    ll, dl = [0] * 286, [0, 0, 0, 1]
    for s, l in ((257, 1), (285, 2), (256, 3), (65, 4), (67, 5), (71, 6), (84, 6)):
        ll[s] = l
    return [Dynamic(list(b"ACGT") + [(3, 4)] * 300 + [(258, 4)] * 30, lit_lens=ll, dist_lens=dl, hdist=4)]


SHORT_LENS = {65: 1, 67: 2, 71: 3, 84: 4, 256: 5, 78: 5}


def _case_short_literals():
    ll = [0] * 286
    for s, l in SHORT_LENS.items():
        ll[s] = l
    rng = np.random.default_rng(12)
    blocks = []
    for s in range(64):
        body = bytes(rng.choice(np.frombuffer(b"ACG", dtype=np.uint8), p=[.4, .35, .25], size=150))
        blocks.append(Dynamic(list(b"A" * s + body + b"T"), lit_lens=ll, dist_lens=[0], hlit=257, hdist=1))
    return blocks


def _case_chain():
    tok = list(b"ACGTACGG") + [(8, 8)] * 64 + list(b"TTGCA") + [(16, 5)] * 64
    for d in (2, 3, 7, 63):
        tok += list(_acgt(70, d)) + [(258, d)]
    return [Dynamic(tok + list(_acgt(2600, 3)))]


def _case_stored_alignments():
    blocks = []
    for k in range(8):
        blocks += [Fixed(list(b"ACGT") + [(11, 1)] * k), Stored(b"ACGTACGT")]      # a fixed block of 42 + 13 k bits: every alignment
    blocks += [Dynamic(list(_acgt(300, 1))), Stored(b""), Dynamic(list(_acgt(300, 2))), Stored(b"A"), Stored(b""), Fixed([]), Dynamic([])]
    return blocks


def _case_headers():
    # a run of equal lengths over the HLIT / HDIST boundary (repeat 16), zeros in runs of 138 (repeat 18), sixteen distance codes
    ll = [0] * 258
    for s, l in ((65, 2), (67, 2), (71, 2), (84, 3), (256, 4), (257, 4)):
        ll[s] = l
    b = Dynamic(list(_acgt(40, 5)) + [t for d in range(1, 30, 2) for t in list(_acgt(6, d)) + [(3, d)]], lit_lens=ll, dist_lens=[4] * 16)
    assert (18, 127) in b.cl_syms and b.cl_syms[-4:] == [(4, 0), (16, 3), (16, 3), (16, 2)], b.cl_syms[-6:]
    return [b]


def _case_hclen_5():
    # HCLEN = 5: lengths for the code-length symbols 16 17 18 0 8 only -- 256 literal/length codes of eight bits, no distance code
    cl = [0] * 19
    cl[8], cl[0], cl[18], cl[17] = 1, 2, 3, 3
    ll = [8] * 255 + [0, 8]
    rng = np.random.default_rng(8)
    return [Dynamic([int(v) for v in rng.integers(0, 255, size=300)], lit_lens=ll, dist_lens=[0], hlit=257, hdist=1,
                    cl_syms=[(8, 0)] * 255 + [(0, 0), (8, 0), (0, 0)], cl_lens=cl, hclen=5)]


R_BIG, BACK = 313, 96       # record length and how many records back the far matches of big_member reach (30 048 bytes)


def _case_big():
    """> 200 KiB of DEFLATE bytes: twelve blocks of 100 records -- dynamic with two distance codes (complete: a block start the search
    can propose), dynamic with one, fixed, stored -- every fourth quality line a match 30 048 bytes back, over every block boundary"""
    h = _hap().upper().replace(b"N", b"A")
    rng = np.random.default_rng(21)
    text, blocks, tok = bytearray(), [], []
    kinds = ["two", "one", "two", "fixed", "two", "stored"] * 2
    for k in range(100 * len(kinds)):
        kind = kinds[k // 100]
        s = int(rng.integers(0, len(h) - 150))
        p = len(text)
        if k >= BACK and k % 4 == 0:
            qual = bytes(text[p - BACK * R_BIG + 162:p - BACK * R_BIG + 312])
        else:
            qual = bytes((33 + rng.integers(2, 41, size=150)).astype(np.uint8))
        rec = b"@r%06d\n" % k + h[s:s + 150] + b"\n+\n" + qual + b"\n"
        assert len(rec) == R_BIG
        text += rec
        if kind != "stored":
            if kind in ("two", "fixed") and k and text[p:p + 5] == text[p - R_BIG:p - R_BIG + 5]:
                tok += [(5, R_BIG)] + list(rec[5:162])
            else:
                tok += list(rec[:162])
            tok += [(150, BACK * R_BIG), 10] if k >= BACK and k % 4 == 0 else list(rec[162:])
        if k % 100 == 99:
            blocks.append(Stored(text[len(text) - 100 * R_BIG:]) if kind == "stored" else Fixed(tok) if kind == "fixed" else Dynamic(tok))
            if kind == "one":
                assert sum(1 for l in blocks[-1].dist_lens if l) == 1
            if kind == "two":
                assert db.kraft(blocks[-1].dist_lens) == 32768 and db.kraft(blocks[-1].lit_lens) == 32768
            tok = []
    return bytes(text), blocks


def _false_block(as_block=False):
    tok = []
    for i in range(40):
        tok += list(_acgt(60, 50 + i)) + [(5 + i % 20, 1 + (i * 7) % 50), (3, 60)]
    b = Dynamic(tok)
    b.final = False
    if as_block:
        return b
    w = db.BitWriter()
    b.write(w)
    assert db.kraft(b.lit_lens) == db.kraft(b.dist_lens) == 32768
    return w.done()


def _case_trap(at):
    """stored noise whose payload holds a genuine non-final dynamic block at compressed offset `at` of the gzip file (header 10 bytes)"""
    rng = np.random.default_rng(at)
    f = _false_block()
    first = bytearray(rng.integers(0, 256, size=65535, dtype=np.uint8).tobytes())
    o = at - 10 - 5
    first[o:o + len(f)] = f
    blocks = [Stored(first), Stored(rng.integers(0, 256, size=30000, dtype=np.uint8).tobytes())]
    return blocks, at


def _bad_cases():
    """(name, blocks or bytes)"""
    pre = Fixed(list(b"ACGTTGCA" * 12 + b"ACGT"))      # 100 bytes of text in front of what zlib refuses
    A, C = 65, 67

    def ll(**kw):
        v = [0] * 286
        for k, l in kw.items():
            v[{"A": 65, "C": 67, "G": 71, "T": 84, "E": 256, "L": 257}[k]] = l
        return v
    ok_lit = ll(A=1, C=2, E=3, L=3)
    # the code-length code of the same header with its longest code one bit longer (incomplete) / shorter (over-subscribed)
    ref = Dynamic([], lit_lens=ok_lit)
    top = max(range(19), key=lambda s: ref.cl_lens[s])
    assert 2 <= ref.cl_lens[top] < 7
    cl_inc, cl_over = list(ref.cl_lens), list(ref.cl_lens)
    cl_inc[top] += 1
    cl_over[top] -= 1
    toks = [A, C, A, A, C]
    out = [
        ("incomplete_lit", [pre, Dynamic(toks, lit_lens=ll(A=2, C=2, E=2))]),
        ("incomplete_dist", [pre, Dynamic(toks + [(3, 1), (3, 2)], lit_lens=ok_lit, dist_lens=[2, 2])]),
        ("incomplete_dist_three_codes", [pre, Dynamic(toks + [(3, 1)], lit_lens=ok_lit, dist_lens=[1, 2, 3])]),
        ("incomplete_lit_one_long_code", [pre, Dynamic([A, A], lit_lens=ll(A=1, E=2))]),
        ("incomplete_clen", [pre, Dynamic(toks, lit_lens=ok_lit, cl_lens=cl_inc)]),
        ("over_lit", [pre, Dynamic(toks, lit_lens=ll(A=1, C=1, E=1))]),
        ("over_dist", [pre, Dynamic(toks, lit_lens=ok_lit, dist_lens=[1, 1, 1])]),
        ("over_clen", [pre, Dynamic(toks, lit_lens=ok_lit, cl_lens=cl_over)]),
        ("no_eob_code", [pre, Dynamic(toks, lit_lens=ll(A=1, C=1), eob=False)]),
        ("hclen_4_no_eob", [pre, Dynamic([], lit_lens=[0] * 257, hlit=257, hdist=1, cl_syms=[(18, 127), (18, 109)], cl_lens=_cl(18, 0), hclen=4, eob=False)]),
        ("repeat_16_first", [pre, Dynamic(toks, lit_lens=ok_lit, cl_syms=[(16, 0), (0, 0)], cl_lens=_cl(16, 0))]),
        ("hlit_287", [pre, Dynamic(toks, lit_lens=db.FIXED_LIT, dist_lens=[5] * 32, hlit=287, hdist=30)]),
        ("hlit_288", [pre, Dynamic(toks, lit_lens=db.FIXED_LIT, dist_lens=[5] * 32, hlit=288, hdist=30)]),
        ("hdist_31", [pre, Dynamic(toks, lit_lens=db.FIXED_LIT, dist_lens=[5] * 32, hlit=286, hdist=31)]),
        ("hdist_32", [pre, Dynamic(toks, lit_lens=db.FIXED_LIT, dist_lens=[5] * 32, hlit=286, hdist=32)]),
        ("block_type_3", [pre, _RawBlock([Raw(0b110, 3), Raw(0x5A5A, 16)])]),
        ("nlen_mismatch", [pre, Stored(b"ACGTACGT", nlen=0x1234)]),
        ("fixed_sym_286", [pre, Fixed([A, C, Sym(286), A])]),
        ("fixed_sym_287", [pre, Fixed([A, C, Sym(287), A])]),
        ("fixed_dist_30", [pre, Fixed([A, C, Sym(257), DSym(30), A])]),
        ("fixed_dist_31", [pre, Fixed([A, C, Sym(257), DSym(31), A])]),
        ("length_without_distance_code", [pre, Dynamic([A, C, Sym(257), Raw(0, 3)], lit_lens=ok_lit, dist_lens=[0], hdist=1)]),
        ("distance_beyond_text_0", [Fixed([(3, 1), A])]),
        ("distance_beyond_text_100", [pre, Fixed([A, (3, 102), A])]),
        ("distance_beyond_text_32767", [Stored(np.random.default_rng(1).integers(0, 256, size=32767, dtype=np.uint8).tobytes()), Fixed([(3, 32768), A])]),
    ]
    # a repeat that runs past HLIT + HDIST
    b = Dynamic(toks, lit_lens=ok_lit)
    assert b.cl_syms[-1] == (0, 0)
    past = Dynamic(toks, lit_lens=ok_lit, cl_syms=b.cl_syms[:-1] + [(17, 0)])      # three zeros where one length is left
    out.append(("repeat_past_the_end", [pre, past]))
    # a stream cut inside a header, inside a symbol, inside a stored payload
    whole = db.deflate([copy.deepcopy(pre), Dynamic(list(_acgt(200, 4)) + [(30, 50)]), Stored(b"ACGT" * 50)])
    hdr_at = len(db.deflate([copy.deepcopy(pre)]))
    out += [("cut_in_header", whole[:hdr_at + 6]), ("cut_in_symbol", whole[:hdr_at + 60]), ("cut_in_stored", whole[:len(whole) - 77])]
    return out


def _cl(*syms):
    v = [0] * 19
    for s in syms:
        v[s] = 1 if len(syms) <= 2 else 2
    return v


class _RawBlock:
    final = False

    def __init__(self, tokens):
        self.tokens = tokens

    def write(self, w):
        for t in self.tokens:
            w.put(t.value, t.nbits)


class Case:
    def __init__(self, name, body, text, ok, fastq=False, gzip=True, bgzf=True, fields=False, must=True):
        self.name, self.body, self.text, self.ok, self.fastq, self.gzip, self.bgzf, self.fields = name, body, text, ok, fastq, gzip, bgzf, fields
        self.must = must and ok          # the gzip decoder of the device has to decode it whole

    def gz(self):
        return db.gzip_member(self.body, self.text, self.fields)

    def bz(self):
        return db.bgzf_member(self.body, self.text)


_CASES = None


def cases():
    global _CASES
    if _CASES is not None:
        return _CASES
    out = []

    def good(name, blocks, text=None, **kw):
        t = _tokens_text(blocks) if text is None else text
        out.append(Case(name, db.deflate(blocks), t, True, **kw))

    text, blocks = _case_distances()
    good("distances_x_lengths", blocks, text, fastq=True)
    good("distances_x_lengths_fields", copy.deepcopy(blocks), text, fastq=True, bgzf=False, fields=True)
    for kind in ("fixed", "dynamic"):
        text, blocks = _case_all_symbols(kind)
        good("all_symbols_" + kind, blocks, text, fastq=True)
    good("long_codes", _record(_case_long_codes()), fastq=True)
    dense = _record(_case_dense())
    good("dense_matches", dense, fastq=True, gzip=False)
    t = _tokens_text(dense)
    noise = np.random.default_rng(2).integers(0, 256, size=len(t) // 7 + 64, dtype=np.uint8).tobytes()
    good("dense_matches_padded", [Stored(noise)] + copy.deepcopy(dense))
    good("short_literal_runs", _record(_case_short_literals()), fastq=True)
    good("match_chains", _record(_case_chain()), fastq=True)
    good("stored_alignments", _record(_case_stored_alignments(), tail=[Stored(b"")]), fastq=True)
    good("dynamic_headers", _record(_case_headers()), fastq=True)
    good("hclen_5", _case_hclen_5())
    good("fixed_every_byte", [Fixed(list(range(256)))])
    big = np.random.default_rng(6).integers(0, 256, size=65535, dtype=np.uint8).tobytes()
    good("stored_0_1_65535", [Stored(b""), Stored(b"x"), Stored(big), Stored(b"")], bgzf=False)
    text, blocks = _case_big()
    good("big_member", blocks, text, fastq=True, bgzf=False)
    for name, at in (("trap_at_48k", SEG), ("trap_behind_48k", SEG + 776)):
        blocks, _ = _case_trap(at)
        good(name, blocks, bgzf=False, must=False)
    for name, b in _bad_cases():
        body = b if isinstance(b, bytes) else db.deflate(b)
        text, ok = zlib_prefix(body)
        assert not ok, name
        out.append(Case(name, body, text, False))
    _CASES = out
    return out


def by_name(name):
    return next(c for c in cases() if c.name == name)


# ---- the tests ------------------------------------------------------------------------------------------------------------------
def test_builder_and_zlib_agree_on_every_conformant_case():
    names = [c.name for c in cases()]
    assert len(set(names)) == len(names)
    for c in cases():
        got, ok = zlib_prefix(c.body)
        assert ok == c.ok, c.name
        assert got == c.text, c.name
        if c.ok:
            d = zlib.decompressobj(-15)
            assert d.decompress(c.body) == c.text and d.eof and d.unused_data == b"", c.name
    assert sum(c.ok for c in cases()) >= 17 and sum(not c.ok for c in cases()) >= 29


def test_what_zlib_refuses_and_why():
    """the error each non-conformant case is there for (zlib's own words), so that a case cannot rot into another error"""
    want = {"incomplete_lit": "invalid literal/lengths set", "incomplete_lit_one_long_code": "invalid literal/lengths set",
            "incomplete_dist": "invalid distances set", "incomplete_dist_three_codes": "invalid distances set",
            "incomplete_clen": "invalid code lengths set", "over_lit": "invalid literal/lengths set", "over_dist": "invalid distances set",
            "over_clen": "invalid code lengths set", "no_eob_code": "missing end-of-block", "hclen_4_no_eob": "missing end-of-block",
            "repeat_16_first": "invalid bit length repeat", "repeat_past_the_end": "invalid bit length repeat",
            "hlit_287": "too many length or distance symbols", "hlit_288": "too many length or distance symbols",
            "hdist_31": "too many length or distance symbols", "hdist_32": "too many length or distance symbols",
            "block_type_3": "invalid block type", "nlen_mismatch": "invalid stored block lengths",
            "fixed_sym_286": "invalid literal/length code", "fixed_sym_287": "invalid literal/length code",
            "fixed_dist_30": "invalid distance code", "fixed_dist_31": "invalid distance code",
            "length_without_distance_code": "invalid distance code", "distance_beyond_text_0": "invalid distance too far back",
            "distance_beyond_text_100": "invalid distance too far back", "distance_beyond_text_32767": "invalid distance too far back"}
    for c in cases():
        if c.ok:
            continue
        try:
            zlib.decompressobj(-15).decompress(c.body)
            msg = "cut"
        except zlib.error as e:
            msg = str(e)
        if c.name.startswith("cut_"):
            assert msg == "cut", (c.name, msg)
        else:
            assert want[c.name] in msg, (c.name, msg)
    # what zlib accepts (the other side of the same line): one distance code, 15-bit codes, 284 + 31, distance 32 768
    assert by_name("dense_matches").ok and by_name("long_codes").ok and by_name("distances_x_lengths").ok


def test_case_conditions():
    for c in cases():
        if c.must and c.gzip:
            assert len(c.text) <= 8 * len(c.body), (c.name, len(c.text), len(c.body))      # else the device may hand it to the host (kGzRatio)
            assert len(c.gz()) >= 64, c.name
        if c.bgzf:
            assert len(c.text) <= 65536 and len(c.bz()) <= 65536, c.name
        if c.fastq:
            lines = c.text.split(b"\n")
            assert lines[-1] == b"" and len(lines) % 4 == 1, c.name
            assert all(a[:1] == b"@" and p == b"+" and len(s) == len(q) and len(s) > 0
                       for a, s, p, q in zip(lines[0:-1:4], lines[1::4], lines[2::4], lines[3::4])), c.name
    big = by_name("big_member")
    assert len(big.body) > 200 << 10
    # runs of three short literals start at bits 61, 62 and 63 of a 64-bit sub-block, counted from a block's first symbol
    seen = set()
    for b in _case_short_literals():
        pos, lens = 0, [SHORT_LENS[t] for t in b.tokens]
        for i, l in enumerate(lens[:-3]):
            if pos % 64 >= 61 and lens[i] + lens[i + 1] + lens[i + 2] <= 10:
                seen.add(pos % 64)
            pos += l
    assert seen == {61, 62, 63}
    # the dense block: more than 192 matches in its first 4096 bits, more than 1536 bytes from 64 bits of the long ones
    assert 4096 // 2 > 192 and 300 > 192 and (64 // 3) * 258 > 1536
    # the traps: a block start the search accepts stands where it looks first
    for name, at in (("trap_at_48k", SEG), ("trap_behind_48k", SEG + 776)):
        gz = by_name(name).gz()
        f = _false_block()
        assert gz[at:at + len(f)] == f and at % 8 == 0 and len(gz) * 8 - at * 8 > 2048 + 8 * len(f)
        whole = db.deflate([_false_block(True), Stored(b"")])      # a genuine block: zlib decodes it (an empty last block behind it)
        d = zlib.decompressobj(-15)
        assert whole[:len(f) - 1] == f[:-1] and len(d.decompress(whole)) > 2000 and d.eof


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("inflate_shapes") / "inflate_check")
    cmd = ["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-std=c++17", "-I", HOST,
           os.path.join(ROOT, "tests", "native", "inflate_check.cpp"), os.path.join(HOST, "fast_inflate.cpp"), "-lz", "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return exe


def test_host_decoder_agrees_with_zlib_on_every_case(driver, tmp_path):
    paths = []
    for c in cases():
        p = tmp_path / (c.name + ".gz")
        p.write_bytes(c.gz())
        paths.append(str(p))
    r = subprocess.run([driver] + paths, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert f"{len(paths)} files, 0 mismatches" in r.stdout
