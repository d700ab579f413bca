"""Reads and key sets for the even-k tests of the device-side readers (test_gpu_even_k_readers.py, test_gpu_even_k_product.py).

Even k is history-dependent in the reference (src/kmer.cpp:132-146): the run counter l is not advanced on a window that is its own
reverse complement -- of the REGISTERS' content, stale bases from in front of a non-base and the zeros in front of the read included --
so behind such a window the positions with  run of bases >= k > l  are not emitted.  The reads built here meet that in every way the
debit pass and the exact tail have to get right, and the key set HOLDS the suppressed windows (the same reads sketched from other start
offsets), so that a kernel which counts them is caught.  Expected counters always come from the oracle's literal state machine."""
import functools

import numpy as np

import oracle_lib as o

_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
_COMP = {65: 84, 67: 71, 71: 67, 84: 65}
_CODE = {65: 0, 67: 1, 71: 2, 84: 3}

# name: (k, more than 65 536 keys)
TABLES = {"k22-path-table": (22, False), "k26-context-table": (26, False), "k28-context-table": (28, False),
          "k22-context-table-by-id": (22, True), "k16-literal": (16, False)}


class Case:
    pass


def fastq(reads, qual_seed=None):
    """four-line records; qual_seed: qualities drawn at random (a read set of repeats with constant qualities compresses past what the
    device's gzip decoder has room for per compressed byte, and it then hands the stream to the host: not what a sequencer writes)"""
    if qual_seed is None:
        return b"".join(b"@r%d/1 x\n%s\n+\n%s\n" % (i, r, b"I" * len(r)) for i, r in enumerate(reads))
    rng = np.random.default_rng(qual_seed)
    return b"".join(b"@r%d/1 x\n%s\n+\n%s\n" % (i, r, rng.integers(35, 75, size=len(r), dtype=np.uint8).tobytes()) for i, r in enumerate(reads))


def fasta(reads, width=60):
    return b"".join(b">r%d x\n" % i + b"".join(r[p:p + width] + b"\n" for p in range(0, len(r), width)) for i, r in enumerate(reads))


def block_of(reads):
    return np.frombuffer(b"".join(r + b"\n" for r in reads), dtype=np.uint8)


def expected(case, reads):
    t = o.Table(case.keys)
    t.count_block(block_of(reads), case.k)
    return t.counts()


@functools.lru_cache(maxsize=None)
def make(name):
    k, big = TABLES[name]
    rng = np.random.default_rng(1000 + k + (7 if big else 0))

    def rnd(n):
        return _ACGT[rng.integers(0, 4, size=n)].tobytes()

    pals = []

    def own_rc():      # a k-mer that is its own reverse complement
        h = rnd(k // 2)
        pals.append(h + bytes(_COMP[b] for b in reversed(h)))
        return pals[-1]

    genome = rnd(2400)
    specials = []
    for i in range(14):
        body = genome[40 * i:40 * i + 100]
        specials += [
            b"T" * (k // 2) + body,                                        # the phantom window A^(k/2) T^(k/2) of the zeroed registers
            own_rc() + body,                                               # starts with its own reverse complement
            body[:30] + b"N" + own_rc() + body[30:],                       # the same behind an N (stale bases in the registers)
            own_rc() + own_rc() + body,                                    # two of them in a row
            body[:30] + b"NN" + own_rc() + body[30:],                      # NN
            body[:20] + b"N" + own_rc()[:5] + b"n" + own_rc() + body[20:],   # two non-bases within k bases of each other
            b"N" + own_rc() + body,                                        # a non-base as the first byte of a read
            body + b"N",                                                   # ... and as the last
            own_rc()[:k - 1] + b"N" + body,
            body[:40] + b"N" + b"T" * (k // 2 - 3) + body[40:],
            (body[:30] + b"N" + own_rc() + body[30:]).lower(),             # lower-case reads
            (own_rc() + body).lower(),
            body[:35] + b"." + own_rc()[1:] + body[35:],
        ]
    plain = [genome[s:s + 120] for s in rng.integers(0, len(genome) - 120, size=500)]
    hot = [genome[1000:1140]] * 300                                        # counters past the clamp
    keysets = [o.sketch(r, k) for r in specials] + [o.sketch(r[1:], k) for r in specials] + [o.sketch(b"G" + r, k) for r in specials] + [o.sketch(genome, k)]
    keys = np.unique(np.concatenate(keysets))
    keys = keys[keys != np.uint64(0xFFFFFFFFFFFFFFFF)]
    # the k-mers that are their own reverse complement as keys too: the reference never emits them, their counters stay zero
    from varigraph_amd import synth
    pal_codes = np.array([sum(_CODE[b] << (2 * (k - 1 - i)) for i, b in enumerate(q)) for q in pals[:40]], dtype=np.uint64)
    keys = np.unique(np.concatenate([keys, (synth.hash64_np(pal_codes, k) << np.uint64(8)) | np.uint64(k)]))
    if big:
        keys = np.unique(np.concatenate([keys, o.sketch(rnd(90_000), k)]))
        keys = keys[keys != np.uint64(0xFFFFFFFFFFFFFFFF)]
        assert keys.size > 65536
    else:
        assert 1000 < keys.size <= 65536
    reads = specials * 12 + plain + hot
    reads = [reads[i] for i in rng.permutation(len(reads))]
    c = Case()
    c.name, c.k, c.big, c.keys, c.reads, c.specials, c.genome = name, k, big, keys, reads, specials, genome
    c.own_rc = pals
    c.want = expected(c, reads)
    # (checked on the CPU before the parameters were fixed, and asserted by the tests: counters at the clamp and below it)
    assert (c.want == 255).any() and (c.want < 255).any()
    return c


def fit(case, head, total):
    """reads whose '\\n'-joined block is exactly `total` bytes: `head`, then slices of the genome, the last one cut to fit"""
    reads, size, i = list(head), sum(len(r) + 1 for r in head), 0
    assert size <= total and total - size != 1
    while size < total:
        room = total - size - 1
        n = min(110, room)
        if room - n == 1:      # (what is left must hold a base and its '\n')
            n -= 1
        s = (37 * i) % (len(case.genome) - 110)
        reads.append(case.genome[s:s + n])
        size += n + 1
        i += 1
    assert size == total
    return reads
