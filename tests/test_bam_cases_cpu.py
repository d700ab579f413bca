"""The hand-built BAM streams of tests/bam_cases.py are what they claim: the host decoder (vgh_bam_read_all) reads every one as the
Python model does, or names the expected byte; and, by the candidate rule restated in bam_cases.candidates, every planted fake is a
false candidate where the case says so, none lies on the true chain, and the walk from one yields other reads than the true walk --
so a device that links or marks a chain wrongly cannot pass tests/test_gpu_bam_cases.py."""
import zlib

import pytest

import bam_cases as K
import bam_py as B
from varigraph_amd import host


@pytest.mark.parametrize("name", K.names())
def test_host_decoder_equals_the_model(name, tmp_path):
    c = K.get(name)
    p = tmp_path / "c.bam"
    p.write_bytes(c.comp)
    if c.error_what:
        with pytest.raises(RuntimeError) as e:
            host.bam_read_all(str(p))
        assert str(e.value) == c.error(p)
    else:
        block, n, rb = host.bam_read_all(str(p), decode_threads=2)
        assert (block.tobytes(), n, rb) == B.reads_block(c.recs)
    # the members are stored, a chunk's members hold that chunk's bytes, and `piece` commits them chunk by chunk
    pos = at = 0
    for (a, e), n_comp in zip(c.chunks(), c.piece):
        text = b""
        end = pos + n_comp
        while pos < end and c.comp[pos:pos + 28] != B.BGZF_EOF:
            total = int.from_bytes(c.comp[pos + 16:pos + 18], "little") + 1
            assert c.comp[pos + 18] == 1 and total == 31 + c.sizes[at]          # one final stored block
            text += zlib.decompress(c.comp[pos:pos + total], 31)
            pos += total
            at += 1
        assert text == c.raw[a:e], (name, a, e)
    assert c.comp[pos:] == B.BGZF_EOF


def _cands(c, lo=None, end=None):
    return K.candidates(c.raw, c.hlen if lo is None else lo, len(c.raw) if end is None else end, c.n_ref)


@pytest.mark.parametrize("name", [n for n in K.names() if K._BUILDERS[n][0] != "capacity"])
def test_candidates_are_the_records_and_the_planted_fakes(name):
    c = K.get(name)
    cands = _cands(c)
    true = [o for i, o in enumerate(c.offs) if i not in c.not_cand]
    false = sorted(o for o, is_cand, _ in c.fakes if is_cand)
    assert cands == sorted(true + false), name
    # no fake on the true chain, whose walk is the model's
    block, n, stop = K.walk(c.raw, c.hlen, len(c.raw), c.n_ref)
    assert (block, n, stop) == (c.block, c.n_records, c.consumed)
    assert not {o for o, _, _ in c.fakes} & set(c.offs)
    for idx, n_inside in c.inside.items():
        end = c.offs[idx] + 4 + int.from_bytes(c.raw[c.offs[idx]:c.offs[idx] + 4], "little")
        assert sum(c.offs[idx] < o < end for o in false) == n_inside, (name, idx)
    # the wrong walk: entering a fake yields a read the true chain does not have
    for o, is_cand, r in c.fakes:
        wrong, n_wrong, _ = K.walk(c.raw, o, len(c.raw), c.n_ref)
        if is_cand:
            assert n_wrong >= 1 and wrong.startswith(r.seq + b"\n") and r.seq + b"\n" not in c.block
            before = B.reads_block([q for q, qo in zip(c.recs, c.offs) if qo < o])[0]
            assert before + wrong != B.reads_block(c.recs)[0][:len(before + wrong)]
        else:
            assert n_wrong == 0
    if c.n_cand is not None:
        assert len(cands) == c.n_cand and len(c.chunks()) == 1


def test_families():
    want = {"planted": 15, "sweep": 2 * len(K.SWEEP) + 4, "seqlen": 3, "carry": 4, "chain": len(K.CHAIN_LENS) + 7, "nref": 2,
            "malformed": len(K.ERRORS) * 6, "capacity": 1}
    assert {f: len(K.names(f)) for f in K.families()} == want


def _link_distance(c, idx):
    """candidates between a true record and its successor: what bam_link_kernel's probe and search step over"""
    cands = _cands(c)
    return cands.index(c.offs[idx + 1]) - cands.index(c.offs[idx]) - 1 if idx + 1 < len(c.offs) else len(cands) - cands.index(c.offs[idx]) - 1


def test_binary_search_and_probe_edge():
    for name in K.names("planted"):
        c = K.get(name)
        if name.startswith("binary_search"):
            assert c.inside[6] >= 5 and _link_distance(c, 6) == c.inside[6]
    assert _link_distance(K.get("binary_search_6_fakes"), 6) == 6
    assert _link_distance(K.get("binary_search_9_fakes_few_behind"), 6) == 9
    assert _link_distance(K.get("binary_search_5_fakes_last_record"), 6) == 5 and len(K.get("binary_search_5_fakes_last_record").recs) == 7
    assert _link_distance(K.get("probe_edge_3_fakes"), 6) == 3 and _link_distance(K.get("probe_edge_4_fakes"), 6) == 4
    # a fake's own successor: a true boundary, another fake, nothing
    c = K.get("fake_runs_into_a_true_boundary")
    o = sorted(o for o, _, _ in c.fakes)[-1]
    assert K.walk(c.raw, o, len(c.raw), c.n_ref)[2] == len(c.raw) and o + 4 + K._ld32(c.raw, o) == c.offs[7]
    c = K.get("fake_runs_into_a_fake")
    o = sorted(o for o, _, _ in c.fakes)
    assert [a + 4 + K._ld32(c.raw, a) for a in o[:2]] == o[1:]
    c = K.get("one_fake")
    o = c.fakes[0][0]
    assert o + 4 + K._ld32(c.raw, o) not in _cands(c)
    c = K.get("fake_past_the_data")
    o = [o for o, is_cand, _ in c.fakes if not is_cand][0]
    assert o + 4 + K._ld32(c.raw, o) > len(c.raw)
    c = K.get("one_fake_in_qualities")
    r = c.recs[6]
    q0 = c.offs[6] + 36 + len(r.name) + 1 + 4 * len(r.cigar) + (len(r.seq) + 1) // 2
    assert q0 <= c.fakes[0][0] < q0 + len(r.seq) and not r.aux
    for name, flag in (("fakes_in_a_secondary", 0x100), ("fakes_in_a_supplementary", 0x800)):
        assert K.get(name).recs[6].flag & flag and not K.get(name).recs[6].kept
    assert not K.get("fakes_in_a_record_without_sequence").recs[6].seq


def _linked_walk(c, probe=4, search_from=None, search=True):
    """The reads of the chain as bam_link_kernel links it, in a model with its two steps adjustable: the successor of candidate i is
    looked for among the `probe` candidates behind it, then by a search of the candidates from i + 1 + search_from on."""
    cands = _cands(c)
    search_from = probe if search_from is None else search_from
    i, taken = 0, []
    while i is not None:
        o = cands[i]
        taken.append(o)
        nx, j = o + 4 + K._ld32(c.raw, o), None
        for q in range(i + 1, min(i + 1 + probe, len(cands))):
            if cands[q] >= nx:
                j = q if cands[q] == nx else None
                break
        else:
            rest = cands[i + 1 + search_from:] if search else []
            j = i + 1 + search_from + rest.index(nx) if nx in rest else None
        i = j
    return taken


def test_the_planted_cases_tell_a_wrong_link_from_the_right_one():
    """what each case is for, shown on a model of the link step: without the search the chains of the binary-search cases and of the
    4-fakes case end early, a probe one step short loses the 3-fakes case, a search that starts one candidate late the 4-fakes case"""
    for name in K.names("planted"):
        c = K.get(name)
        if len(c.chunks()) == 1:
            assert _linked_walk(c) == c.offs, name
    for name in [n for n in K.names("planted") if n.startswith("binary_search")] + ["probe_edge_4_fakes"]:
        assert _linked_walk(K.get(name), search=False) == K.get(name).offs[:7], name
    assert _linked_walk(K.get("probe_edge_3_fakes"), search=False) == K.get("probe_edge_3_fakes").offs
    assert _linked_walk(K.get("probe_edge_3_fakes"), probe=3, search=False) == K.get("probe_edge_3_fakes").offs[:7]
    assert _linked_walk(K.get("probe_edge_4_fakes"), search_from=5) == K.get("probe_edge_4_fakes").offs[:7]
    assert _linked_walk(K.get("binary_search_6_fakes"), search_from=5) == K.get("binary_search_6_fakes").offs
    # pointer doubling: rounds r = 0, 1, .. while 2^r < n mark 2^rounds nodes; every chain length but 1 loses records to a round too few
    for n in K.CHAIN_LENS:
        rounds = sum(1 for r in range(32) if (1 << r) < n)
        assert (1 << rounds) >= n and (n == 1 or (1 << (rounds - 1)) < n)
    assert {255, 256, 257} <= set(K.CHAIN_LENS)      # 2^r - 1, 2^r, 2^r + 1: 257 takes a round more than the other two


def test_fakes_at_a_chunk_end_and_in_the_carried_tail():
    c = K.get("fakes_in_a_chunks_last_record")
    (a, e), _ = c.chunks()
    assert e == c.offs[7] and all(o in _cands(c, end=e) for o, _, _ in c.fakes)
    c = K.get("fakes_in_the_carried_tail")
    (a, e), _ = c.chunks()
    first = _cands(c, end=e)
    assert c.offs[6] < e < c.offs[7] and c.offs[6] not in first and all(o in first for o, _, _ in c.fakes) and len(c.fakes) == 6
    # ... and again in the next chunk, which starts with the carried record
    second = _cands(c, lo=c.offs[6])
    assert second[0] == c.offs[6] and all(o in second for o, _, _ in c.fakes)


def test_sweep_covers_every_alignment():
    for suffix in ("", "_fakes"):
        seen = set()
        for name in K.names("sweep"):
            if not name.startswith("sweep_") or name.endswith("_fakes") != bool(suffix):
                continue
            c = K.get(name)
            (a, e), _ = c.chunks()
            r = c.offs[6]
            assert c.raw[r + 12] == 4 and c.raw[r + 16] == c.raw[r + 17] == 0 and c.recs[6].kept       # SEQ starts at byte 40
            assert e < K.B.STORED_MAX and len(c.sizes) == 2                                             # one member per commit
            seen.add(r - e)
            if suffix:
                near = [o for o, _, _ in c.fakes]
                assert len(near) == 4 and min(abs(o - e) for o in near) < 120 and c.offs[6] in [o + 4 + K._ld32(c.raw, o) for o in near]
        assert seen == set(range(-44, 9))
    h = K.get("header_ends_with_a_chunk")
    assert h.chunks()[0][1] == h.hlen
    assert K.get("header_ends_a_byte_short_of_a_chunk").chunks()[0][1] == h.hlen + 1
    assert K.get("chunk_ends_a_byte_short_of_the_header").chunks()[0][1] == h.hlen - 1
    c = K.get("header_spans_three_chunks")
    assert len(c.chunks()) == 3 and c.chunks()[1][1] < c.hlen


def test_sequence_length_cases():
    for k in (27, 11, 22):
        c = K.get("seqlen_k%d" % k)
        for flag in (0, 16):
            lens = [len(r.seq) for r in c.recs if r.flag == flag]
            assert set(K.SEQ_LENS(k)) <= set(lens)
            assert {1, 255} <= {len(r.name) + 1 for r in c.recs if r.flag == flag}
            assert {0, 65535} <= {len(r.cigar) for r in c.recs if r.flag == flag}
            assert any(r.aux for r in c.recs if r.flag == flag)
        # the padding nibble really is in the stream, and every code sits in both nibbles
        i = [r.name for r in c.recs].index(b"pad")
        r = c.recs[i]
        assert len(r.seq) % 2 and c.raw[c.offs[i] + 36 + 4 + (len(r.seq) + 1) // 2 - 1] & 15 == 15
        i = [r.name for r in c.recs].index(b"codes")
        r = c.recs[i]
        body = c.raw[c.offs[i] + 36 + 6:c.offs[i] + 36 + 6 + (len(r.seq) + 1) // 2]
        assert {b >> 4 for b in body} == {b & 15 for b in body} == set(range(16))
        assert len(c.chunks()) > 4


def test_carry_limit_records():
    for name in K.names("carry"):
        c = K.get(name)
        bs = K._ld32(c.raw, c.offs[5])
        assert bs == (K.TAIL_MAX - 4 if "taken" in name else K.TAIL_MAX - 3)
        assert (c.stop, c.stopped) == ((None, False) if "taken" in name else (5, True))
        assert len(c.chunks()) == (2 if "split" in name else 1)
        if "split" in name:
            assert c.offs[5] < c.chunks()[0][1] < c.offs[6]
    assert _cands(K.get("carry_limit_taken_whole")).count(K.get("carry_limit_taken_whole").offs[5]) == 1


def test_chain_cases():
    for n in K.CHAIN_LENS:
        assert len(K.get("chain_%d" % n).recs) == n
    assert K.get("chain_4_none_kept").n_records == 0 and K.get("chain_4_none_kept").block == b""
    assert len(K.get("chain_30000").recs) >= 30000 and len(K.get("chain_30000").chunks()) == 1
    c = K.get("chain_chunks_of_1_2_3_4_5")
    assert [len(_cands(c, lo=max(a, c.hlen), end=e)) for a, e in c.chunks()] == [1, 2, 3, 4, 5]
    assert all(1 <= len(r.seq) <= 3 for r in c.recs)


def test_malformed_cases_cover_every_class_and_place():
    for what in K.ERRORS:
        for place in ("first", "middle", "later"):
            for fake in ("", "_fake"):
                c = K.get("malformed_%s_%s%s" % (what, place, fake))
                assert c.stop == (0 if place == "first" else 4) and len(c.fakes) == bool(fake)
                if place == "later":      # the bad record arrives through the carry
                    assert c.offs[c.stop] < c.chunks()[0][1] < c.offs[c.stop] + 24
                if fake:                  # inside what the bad record was before the damage
                    assert c.offs[c.stop] < c.fakes[0][0] < c.offs[c.stop + 1]
    assert K._s32(K.get("malformed_ref_hi_middle").raw, K.get("malformed_ref_hi_middle").offs[4] + 4) == 2
    assert K._s32(K.get("malformed_next_lo_middle").raw, K.get("malformed_next_lo_middle").offs[4] + 24) == -2


def test_capacity_case_exceeds_the_candidate_arrays():
    c = K.get("more_candidates_than_the_arrays_hold")
    assert K._ld32(c.raw, c.offs[5]) == K.TAIL_MAX - 4
    # chunks of one stored member each: the last chunk end inside the record
    e = c.offs[6] // B.STORED_MAX * B.STORED_MAX
    assert c.offs[5] < B.STORED_MAX and e > c.offs[5]
    n = len(K.candidates(c.raw, c.offs[5], e, c.n_ref))
    print("candidates in the carry and chunk ending at byte", e, ":", n, "capacity", K.CAP_CAND)
    assert n > K.CAP_CAND
    # none of them a read: what the device must not take changes nothing the host would count
    o = K.candidates(c.raw, c.offs[5], c.offs[5] + 200_000, c.n_ref)
    assert o[1] - o[0] == 16 and K._ld32(c.raw, o[0]) == 65536 and K._ld32(c.raw, o[0] + 20) == 0
