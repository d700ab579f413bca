"""A small DEFLATE (RFC 1951) writer in plain Python, for streams no compressor would write: a list of blocks -- stored bytes, fixed
codes + tokens, dynamic codes + tokens with every header field open to the caller -- becomes a bit-exact body; gzip_member /
bgzf_member wrap it (RFC 1952, SAM spec 4.1).  A helper of the tests (test_deflate_shapes_cpu.py, test_gpu_deflate_shapes.py).

Tokens: an int is a literal byte; (length, distance) a match; (258, distance, True) the same match written as length symbol 284
with extra bits 31 (legal, never written by zlib); Sym(s) / DSym(s) a bare code of the literal/length / distance alphabet and
Raw(value, nbits) bare bits, for streams that must NOT decode.  A whole code goes out per call, never bit by bit."""
import bisect
import heapq
import struct
import zlib

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289,
             16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32

# length 3..258 -> (symbol, extra bits, extra value); symbol 285 for 258
_LEN_SYM = {}
for _s in range(28):
    for _x in range(1 << LEN_EXTRA[_s]):
        _LEN_SYM[LEN_BASE[_s] + _x] = (257 + _s, LEN_EXTRA[_s], _x)
_LEN_SYM[258] = (285, 0, 0)


def dist_sym(d):
    s = bisect.bisect_right(DIST_BASE, d) - 1
    return s, DIST_EXTRA[s], d - DIST_BASE[s]


class Sym:
    def __init__(self, s):
        self.s = s


class DSym:
    def __init__(self, s):
        self.s = s


class Raw:
    def __init__(self, value, nbits):
        self.value, self.nbits = value, nbits


class BitWriter:
    def __init__(self):
        self.out = bytearray()
        self.acc = 0
        self.n = 0

    def put(self, v, k):
        self.acc |= v << self.n
        self.n += k
        if self.n >= 64:
            self.out += (self.acc & 0xFFFFFFFFFFFFFFFF).to_bytes(8, "little")
            self.acc >>= 64
            self.n -= 64

    def bit_len(self):
        return 8 * len(self.out) + self.n

    def align(self):
        self.put(0, -self.bit_len() % 8)

    def raw_bytes(self, b):
        assert self.bit_len() % 8 == 0
        self.out += self.acc.to_bytes(self.n // 8, "little")
        self.acc = self.n = 0
        self.out += b

    def done(self):
        self.align()
        return bytes(self.out) + self.acc.to_bytes(self.n // 8, "little")


def canon(lens):
    """code lengths -> (bit-reversed code, length) per symbol, RFC 1951 3.2.2 (an over-subscribed set wraps around: it is never decoded)"""
    count = [0] * 17
    for l in lens:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * 17, 0
    for l in range(1, 16):
        code = (code + count[l - 1]) << 1
        nxt[l] = code
    out = []
    for l in lens:
        if not l:
            out.append(None)
            continue
        c = nxt[l] & ((1 << l) - 1)
        nxt[l] += 1
        out.append((int(format(c, "0%db" % l)[::-1], 2), l))
    return out


def kraft(lens):
    """sum of 2^(15 - l): 32768 = complete"""
    return sum(32768 >> l for l in lens if l)


def huff_lengths(freqs, limit):
    """code lengths of a Huffman code for freqs (0: unused) no longer than limit: frequencies are flattened until the tree fits"""
    used = [i for i, f in enumerate(freqs) if f]
    lens = [0] * len(freqs)
    if len(used) == 1:
        lens[used[0]] = 1
        return lens
    f = {i: freqs[i] for i in used}
    while used:
        heap = [(w, i, (i,)) for i, w in f.items()]
        heapq.heapify(heap)
        depth = dict.fromkeys(used, 0)
        tie = len(freqs)
        while len(heap) > 1:
            a, b = heapq.heappop(heap), heapq.heappop(heap)
            for i in a[2] + b[2]:
                depth[i] += 1
            heapq.heappush(heap, (a[0] + b[0], tie, a[2] + b[2]))
            tie += 1
        if max(depth.values()) <= limit:
            for i, d in depth.items():
                lens[i] = d
            break
        f = {i: (w + 1) // 2 for i, w in f.items()}
    return lens


def rle_lengths(seq):
    """code lengths -> code-length symbols (sym, extra value), with repeats 16 / 17 / 18 taken greedily over the whole sequence (and so
    over the HLIT / HDIST boundary, as zlib's do)"""
    out, i, n = [], 0, len(seq)
    while i < n:
        v, j = seq[i], i
        while j < n and seq[j] == v:
            j += 1
        run = j - i
        if v == 0:
            while run >= 11:
                k = min(run, 138)
                out.append((18, k - 11))
                run -= k
            if run >= 3:
                out.append((17, run - 3))
                run = 0
            out += [(0, 0)] * run
        else:
            out.append((v, 0))
            run -= 1
            while run >= 3:
                k = min(run, 6)
                out.append((16, k - 3))
                run -= k
            out += [(v, 0)] * run
        i = j
    return out


class Stored:
    def __init__(self, data, final=False, nlen=None):
        self.data, self.final, self.nlen = bytes(data), final, nlen

    def write(self, w):
        w.put(int(self.final), 1)
        w.put(0, 2)
        w.align()
        n = len(self.data)
        w.put(n, 16)
        w.put((n ^ 0xFFFF) if self.nlen is None else self.nlen, 16)
        w.raw_bytes(self.data)


def _write_tokens(w, tokens, lit, dist, eob):
    put = w.put
    for t in tokens:
        if type(t) is int:
            c = lit[t]
            put(c[0], c[1])
        elif type(t) is tuple:
            length, d = t[0], t[1]
            if len(t) > 2 and t[2]:
                assert length == 258
                s, xb, xv = 284, 5, 31
            else:
                s, xb, xv = _LEN_SYM[length]
            c = lit[s]
            put(c[0] | xv << c[1], c[1] + xb)
            s, xb, xv = dist_sym(d)
            c = dist[s]
            put(c[0] | xv << c[1], c[1] + xb)
        elif isinstance(t, Sym):
            put(*lit[t.s])
        elif isinstance(t, DSym):
            put(*dist[t.s])
        else:
            put(t.value, t.nbits)
    if eob:
        put(*lit[256])


class Fixed:
    def __init__(self, tokens, final=False, eob=True):
        self.tokens, self.final, self.eob = tokens, final, eob

    def write(self, w):
        w.put(int(self.final), 1)
        w.put(1, 2)
        _write_tokens(w, self.tokens, canon(FIXED_LIT), canon(FIXED_DIST), self.eob)


def token_freqs(tokens):
    lit, dist = [0] * 286, [0] * 30
    lit[256] = 1
    for t in tokens:
        if type(t) is int:
            lit[t] += 1
        elif type(t) is tuple:
            lit[284 if len(t) > 2 and t[2] else _LEN_SYM[t[0]][0]] += 1
            dist[dist_sym(t[1])[0]] += 1
    return lit, dist


class Dynamic:
    """lit_lens / dist_lens: the code lengths (default: Huffman codes of the tokens' frequencies, no longer than max_bits); hlit / hdist:
    the header's counts (default: the lists' lengths, trailing zeros cut); cl_syms: the code-length symbols as (symbol, extra value)
    pairs, repeats placed by hand (default: rle_lengths of the two lists run together); cl_lens: the 19 lengths of the code-length
    code (default: a Huffman code of cl_syms, no longer than 7); hclen (default: the fewest that hold cl_lens, 4 at least)."""

    def __init__(self, tokens, final=False, lit_lens=None, dist_lens=None, hlit=None, hdist=None, cl_syms=None, cl_lens=None, hclen=None,
                 max_bits=15, eob=True):
        fl, fd = token_freqs(tokens)
        if lit_lens is None:
            lit_lens = huff_lengths(fl, max_bits)
        if dist_lens is None:
            dist_lens = huff_lengths(fd, max_bits) if any(fd) else [0]
        lit_lens, dist_lens = list(lit_lens), list(dist_lens)
        if hlit is None:
            hlit = max(257, max((i + 1 for i, l in enumerate(lit_lens) if l), default=0))
        if hdist is None:
            hdist = max(1, max((i + 1 for i, l in enumerate(dist_lens) if l), default=0))
        self.lit_lens = (lit_lens + [0] * 288)[:max(hlit, 288)]
        self.dist_lens = (dist_lens + [0] * 32)[:max(hdist, 32)]
        if cl_syms is None:
            cl_syms = rle_lengths(self.lit_lens[:hlit] + self.dist_lens[:hdist])
        if cl_lens is None:
            f = [0] * 19
            for s, _ in cl_syms:
                f[s] += 1
            if sum(1 for x in f if x) < 2:      # (a lone code of one bit is an incomplete set, which zlib refuses here)
                f[0 if f[0] == 0 else 1] += 1
            cl_lens = huff_lengths(f, 7)
        if hclen is None:
            hclen = max(4, max(i + 1 for i in range(19) if cl_lens[CL_ORDER[i]]))
        self.tokens, self.final, self.eob = tokens, final, eob
        self.hlit, self.hdist, self.hclen, self.cl_syms, self.cl_lens = hlit, hdist, hclen, cl_syms, list(cl_lens)

    def write(self, w):
        w.put(int(self.final), 1)
        w.put(2, 2)
        w.put(self.hlit - 257, 5)
        w.put(self.hdist - 1, 5)
        w.put(self.hclen - 4, 4)
        for i in range(self.hclen):
            w.put(self.cl_lens[CL_ORDER[i]], 3)
        cl = canon(self.cl_lens)
        for s, x in self.cl_syms:
            c = cl[s]
            w.put(c[0] | x << c[1], c[1] + (2 if s == 16 else 3 if s == 17 else 7 if s == 18 else 0))
        self.symbols_at = w.bit_len()
        _write_tokens(w, self.tokens, canon(self.lit_lens), canon(self.dist_lens), self.eob)


def deflate(blocks):
    """the blocks one after the other; the last one's BFINAL is set unless any block carries its own"""
    if not any(b.final for b in blocks):
        blocks[-1].final = True
    w = BitWriter()
    for b in blocks:
        b.write(w)
    return w.done()


def expand(tokens, history=b""):
    """the text the tokens stand for (history: text in front of them that matches may reach into)"""
    out = bytearray(history)
    for t in tokens:
        if type(t) is int:
            out.append(t)
        elif type(t) is tuple:
            length, d = t[0], t[1]
            assert 0 < d <= len(out), (d, len(out))
            p = len(out) - d
            if d >= length:
                out += out[p:p + length]
            else:
                for i in range(length):
                    out.append(out[p + i])
    return bytes(out[len(history):])


def gzip_member(body, text, flg_fields=False):
    h = b"\x1f\x8b\x08" + bytes([0x1E if flg_fields else 0]) + b"\0\0\0\0\0\xff"
    if flg_fields:
        h += struct.pack("<H", 7) + b"ab\x03\x00xyz" + b"file.fq\0" + b"a comment\0"
        h += struct.pack("<H", zlib.crc32(h) & 0xFFFF)
    return h + body + struct.pack("<II", zlib.crc32(text), len(text) & 0xFFFFFFFF)


def bgzf_member(body, text):
    total = 18 + len(body) + 8
    assert total <= 65536 and len(text) <= 65536, (total, len(text))
    h = b"\x1f\x8b\x08\x04\0\0\0\0\0\xff" + struct.pack("<H", 6) + b"BC" + struct.pack("<HH", 2, total - 1)
    return h + body + struct.pack("<II", zlib.crc32(text), len(text))


BGZF_EOF = bgzf_member(b"\x03\x00", b"")


def tokenize(text, distances=(), max_len=258, min_len=3, planted=None, history=0):
    """text[history:] as tokens: at a position named in planted ({position: (length, distance)}) that match; else the first of
    `distances` at which at least min_len bytes match, no longer than max_len; else a literal"""
    text = bytes(text)
    n, p, out = len(text), history, []
    planted = planted or {}
    keys = sorted(planted)
    while p < n:
        if p in planted:
            length, d = planted[p][0], planted[p][1]
            assert all(text[p + i] == text[p - d + i] for i in range(length)), (p, length, d)
            out.append(tuple(planted[p]))
            p += length
            continue
        k = bisect.bisect_right(keys, p)
        cap = min(max_len, (keys[k] if k < len(keys) else n) - p)      # (never over the next planted match)
        took = False
        for d in distances:
            if d > p or cap < min_len or text[p:p + min_len] != text[p - d:p - d + min_len]:
                continue
            m = min_len
            while m < cap and text[p + m] == text[p - d + m]:
                m += 1
            out.append((m, d))
            p += m
            took = True
            break
        if not took:
            out.append(text[p])
            p += 1
    return out
