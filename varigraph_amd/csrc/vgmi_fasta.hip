// vgmi_fasta.hip -- FASTA records on the device (gfx950): single-line and wrapped, into the same '\n'-joined read block and the
// same FqState bookkeeping the FASTQ parser (vgmi_fastq.hip) writes, so that the count kernels and the hand-over run unchanged.
//
// Reference behaviour implemented (file:line under the reference tree):
//   kseq_read                     include/kseq.h:192-232   for a stream whose first byte is '>'
//   FastqKmer::fastq_file_open    src/fastq_kmer.cpp:97-105 sequence = ks->seq.s, mReadBase += ks->seq.l
// Line by line, as kseq reads the sequence part of a record (kseq.h:208-215; the first byte of every line decides):
//   '>' or '@'     header line: ends the previous record's sequence and starts a record (:209 ends the loop on either byte, :214 keeps
//                  it as last_char, so the next call takes the line as its header); the rest of the line is passed over whatever
//                  it holds (:201-202)
//   empty          skipped (:210)
//   '+'            kseq turns to quality parsing (:216-226): not FASTA -- the record's header is where the host reader takes over
//   anything else  a sequence line, appended whole (:211-212)
// A record's sequence is the concatenation of its sequence lines and is complete only when the next header line (or the end of
// the data) has been seen.  So of every chunk the records in front of its LAST header line are taken, and everything from that
// header on is carried into the next chunk (up to the 1 MiB carry: a longer record hands the stream over); at the end of the
// data the last record is the unconsumed tail vgmi_fastq_close returns, and the host reader parses it.
// The device stops for good, at the first byte of the record's header line -- a record boundary, where a fresh kseq state is the
// reference's state (the argument of vgmi_fastq.hip's header: kseq is between records there with last_char = 0 and scans to the
// next '>' / '@', this very byte) -- at the first record that has a '+' line, has no sequence byte at all (the reference aborts on
// an empty read, kmer.cpp:124; the host reader says so) or is longer than the carry; and at the chunk's first byte when the chunk
// holds a '\r' or NUL byte (KS_SEP_LINE strips '\r', `string(ks->seq.s)` ends at NUL) or does not start with a header line.
//
// Data flow per chunk (one HIP stream, no host round trip; A1-A3 are vgmi_fastq.hip's K1-K3):
//   A1 newline count per tile -> A2 scan -> A3 newline positions ->
//   A4 every line classified by its first byte; exclusive scan over the lines of (header ? 1 : 0, bytes the line adds to the read
//      block: its length for a sequence line, 1 -- the '\n' that closes the record in front -- for a header line): block sums,
//      A5 scan of the sums, A4 again: per line its offset in the block, per header line its record's number, offset and file
//      position; '+' lines mark their record ->
//   A6 records without a sequence byte, or longer than the carry, marked -> A7 bookkeeping (records, bases, consumed bytes, tail) ->
//   A8 copy of the sequence lines in front of the last accepted record's end, 16 lanes per line (a wrapped line of 60-80 bases is
//      one pass of dword stores), a whole wavefront with 16-byte stores per line of 512 bytes and more -> A9 carry.
// With subsampling (FqBuffers::sub; vgmi_fastq_set_subsample) A4, A7 and A8 are their *_sub forms: a line's record number -- the header
// lines in front of it, a scan of its own -- decides first whether its record is read FqState::n_seen + number of the file and kept;
// the lines of a dropped record and its closing '\n' add nothing to the scanned bytes, so the block closes up over it.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vgmi_subsample.h"
#include "vgmi_block_scan.h"
#include "vgmi_kernels.h"

namespace vgk {

#define FA_NONE 0xFFFFFFFFu
#define FA_LONG 512u                       // a line of this many bytes or more is copied by its whole wavefront

__device__ __forceinline__ uint32_t fa_end(uint32_t tail_max, uint32_t n_new, const uint32_t* n_new_dev)
{
    if (n_new_dev) {
        const uint32_t d = *n_new_dev;
        n_new = d < n_new ? d : n_new;
    }
    return tail_max + n_new;
}

// (uniform) nothing of this chunk is taken: the FASTQ kernels' conditions
__device__ __forceinline__ bool fa_skip(const FqState* st, uint32_t cap_lines) { return st->stopped || st->dirty || st->n_lines > cap_lines; }

// lines of the chunk: one per newline and the unterminated rest behind the last one, if any
__device__ __forceinline__ uint32_t fa_n_lines(const FqState* st, const uint32_t* nlpos, uint32_t end)
{
    const uint32_t n_nl = st->n_lines;
    const uint32_t after = n_nl ? nlpos[n_nl - 1] + 1 : st->start;
    return n_nl + (after < end ? 1u : 0u);
}

// exclusive prefix of a 64-bit value over the block's threads; *total = block sum
__device__ __forceinline__ unsigned long long fa_block_scan_excl(unsigned long long v, unsigned long long* sh, unsigned long long* total)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    unsigned long long inc = v;
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned long long n = __shfl_up(inc, o);
        if (lane >= (uint32_t)o) inc += n;
    }
    if (lane == 63) sh[wave] = inc;
    __syncthreads();
    unsigned long long base = 0, tot = 0;
    for (uint32_t i = 0; i < (blockDim.x >> 6); ++i) {
        if (i < wave) base += sh[i];
        tot += sh[i];
    }
    __syncthreads();
    *total = tot;
    return base + inc - v;
}

// A4: the lines.  Scanned value: high word 1 for a header line, low word the bytes the line adds to the read block.  With e = the
// exclusive prefix of line i: a header line starts record hi(e), whose bases go to packed[lo(e), ...); a sequence line belongs to
// record hi(e) - 1 and goes to packed[lo(e) - 1, ...); the '\n' of record r - 1 is packed[rec_d[r] - 1].
__global__ __launch_bounds__(1024) void fa_lines_kernel(const uint8_t* raw, FqState* st, const uint32_t* nlpos, uint32_t tail_max, uint32_t n_new,
                                                        const uint32_t* n_new_dev, unsigned long long* bsum, uint32_t* dest, uint32_t* rec_d,
                                                        uint32_t* rec_pos, int phase, uint32_t cap_lines)
{
    __shared__ unsigned long long sh[16];
    if (fa_skip(st, cap_lines)) return;
    const uint32_t end = fa_end(tail_max, n_new, n_new_dev);
    const uint32_t L = fa_n_lines(st, nlpos, end);
    if (blockIdx.x * 1024u >= L) return;      // (uniform) the launch is sized for the arrays' capacity
    const uint32_t i = blockIdx.x * 1024u + threadIdx.x;
    uint32_t s = 0, c = '\n';
    unsigned long long v = 0;
    if (i < L) {
        s = i ? nlpos[i - 1] + 1 : st->start;
        const uint32_t e = i < st->n_lines ? nlpos[i] : end;
        if (s < e) c = raw[s];
        if (c == '>' || c == '@') v = (1ull << 32) | 1u;
        else if (c != '+' && c != '\n') v = e - s;
    }
    unsigned long long tot;
    const unsigned long long ex = fa_block_scan_excl(v, sh, &tot);
    if (phase == 0) {
        if (threadIdx.x == 0) bsum[blockIdx.x] = tot;
        return;
    }
    if (i >= L) return;
    const unsigned long long e = bsum[blockIdx.x] + ex;
    const uint32_t hi = (uint32_t)(e >> 32), lo = (uint32_t)e;
    dest[i] = lo - 1u;                        // (a sequence line always follows a header line when line 0 is one: lo >= 1)
    if (v >> 32) {
        if (hi < fasta_cap_rec(cap_lines)) {
            rec_d[hi] = lo;
            rec_pos[hi] = s;
        }
    } else if (c == '+' && hi) {
        atomicMin(&st->first_bad, hi - 1u);
    }
}

// A5: exclusive scan of the live block sums by one workgroup, in place; the total (headers, bytes) goes to *total
__global__ __launch_bounds__(1024) void fa_scan_sums_kernel(const FqState* st, const uint32_t* nlpos, uint32_t tail_max, uint32_t n_new,
                                                            const uint32_t* n_new_dev, unsigned long long* bsum, unsigned long long* total,
                                                            uint32_t cap_lines)
{
    __shared__ unsigned long long sh[16];
    if (fa_skip(st, cap_lines)) {
        if (threadIdx.x == 0) *total = 0;
        return;
    }
    const uint32_t L = fa_n_lines(st, nlpos, fa_end(tail_max, n_new, n_new_dev));
    const uint32_t n = (L + 1023u) / 1024u;
    const uint32_t per = (n + 1023u) / 1024u;
    const uint32_t b = threadIdx.x * per, e = b + per < n ? b + per : n;
    unsigned long long s = 0, tot;
    for (uint32_t i = b; i < e; ++i) s += bsum[i];
    unsigned long long run = fa_block_scan_excl(s, sh, &tot);
    for (uint32_t i = b; i < e; ++i) {
        const unsigned long long x = bsum[i];
        bsum[i] = run;
        run += x;
    }
    if (threadIdx.x == 0) *total = tot;
}

// A6: a complete record (the next header line is in the chunk) without a single sequence byte, or longer than the carry -- wherever
// it lies, so that what the device takes does not depend on where the chunks are cut
__global__ __launch_bounds__(256) void fa_records_kernel(FqState* st, const unsigned long long* total, const uint32_t* rec_d, const uint32_t* rec_pos,
                                                         uint32_t cap_lines, uint32_t tail_max)
{
    if (fa_skip(st, cap_lines)) return;
    const uint32_t n_hdr = (uint32_t)(*total >> 32), H = n_hdr < fasta_cap_rec(cap_lines) ? n_hdr : fasta_cap_rec(cap_lines);
    for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r + 1 < H; r += gridDim.x * blockDim.x)
        if (rec_d[r + 1] == rec_d[r] + 1u || rec_pos[r + 1] - rec_pos[r] > tail_max) atomicMin(&st->first_bad, r);
}

// A7: chunk bookkeeping (one thread) -- before the copy, so that the copy only touches accepted records
__global__ void fa_finish_kernel(const uint8_t* raw, FqState* st, const unsigned long long* total, const uint32_t* rec_d, const uint32_t* rec_pos,
                                 uint32_t n_new, const uint32_t* n_new_dev, uint32_t cap_lines, uint32_t tail_max)
{
    if (threadIdx.x || blockIdx.x) return;
    const uint32_t end = fa_end(tail_max, n_new, n_new_dev);
    uint32_t good = 0, consumed_end = st->start, packed = 0;
    if (!st->stopped && st->start < end) {
        const uint32_t c0 = raw[st->start];
        if (st->dirty || st->n_lines > cap_lines || (c0 != '>' && c0 != '@')) {
            st->stopped = 1;     // nothing of this chunk is taken: the host reader resumes at its first byte
        } else {
            const uint32_t H = (uint32_t)(*total >> 32);     // >= 1: line 0 is a header line; record H - 1 is the one carried
            good = st->first_bad < H - 1u ? st->first_bad : H - 1u;
            if (st->first_bad < H) st->stopped = 1;
            consumed_end = rec_pos[good];
            packed = rec_d[good];
        }
    }
    st->n_good = good;
    st->packed_bytes = packed;
    st->n_records += good;
    st->n_bases += packed - good;
    st->consumed += consumed_end - st->start;
    st->consumed_end = consumed_end;
    uint32_t tail = st->stopped ? 0u : end - consumed_end;
    if (tail > tail_max) {      // a record longer than the carry buffer (a contig, not a read): the host reader's
        st->stopped = 1;
        tail = 0;
    }
    st->tail_len = tail;
}

// the little-endian dword at byte o of raw: two aligned loads (the raw buffer has slack behind the data) and a funnel shift
__device__ __forceinline__ uint32_t fa_ld32(const uint8_t* raw, uint32_t o)
{
    const uint32_t* w = reinterpret_cast<const uint32_t*>(raw + (o & ~3u));
    return __builtin_amdgcn_alignbyte(w[1], w[0], o & 3u);
}

// raw[b, b + len) -> dst[0, len) by `n` lanes (this one is number `l`): bytes up to the destination's W-byte boundary, then aligned
// W-byte stores (W = 4 or 16) fed by funnel-shifted dword loads, then the bytes left over
template <uint32_t W>
__device__ __forceinline__ void fa_copy(const uint8_t* raw, uint32_t b, uint32_t len, uint8_t* dst, uint32_t l, uint32_t n)
{
    uint32_t head = (W - (uint32_t)(reinterpret_cast<uintptr_t>(dst) & (W - 1u))) & (W - 1u);
    head = head < len ? head : len;
    const uint32_t n_w = (len - head) / W, done = head + n_w * W;
    for (uint32_t i = l; i < head; i += n) dst[i] = raw[b + i];
    for (uint32_t w = l; w < n_w; w += n) {
        const uint32_t o = head + w * W;
        if (W == 16u) {
            uint4 x;
            x.x = fa_ld32(raw, b + o);
            x.y = fa_ld32(raw, b + o + 4u);
            x.z = fa_ld32(raw, b + o + 8u);
            x.w = fa_ld32(raw, b + o + 12u);
            *reinterpret_cast<uint4*>(dst + o) = x;
        } else {
            *reinterpret_cast<uint32_t*>(dst + o) = fa_ld32(raw, b + o);
        }
    }
    for (uint32_t i = done + l; i < len; i += n) dst[i] = raw[b + i];
}

// A8: the sequence lines in front of consumed_end -> the read block, and the '\n' behind every accepted record.  Four lines per
// wavefront and step, 16 lanes each; a long line is left to the whole wavefront afterwards.
__global__ __launch_bounds__(256) void fa_pack_kernel(const uint8_t* raw, const FqState* st, const uint32_t* nlpos, const uint32_t* dest,
                                                      const uint32_t* rec_d, uint8_t* packed)
{
    const uint32_t good = st->n_good;
    if (!good) return;
    const uint32_t stop = st->consumed_end, start = st->start, n_nl = st->n_lines;
    const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x, n_thr = gridDim.x * blockDim.x;
    for (uint32_t r = tid + 1; r <= good; r += n_thr) packed[rec_d[r] - 1u] = '\n';
    const uint32_t lane = threadIdx.x & 63u, sub = lane >> 4, l16 = lane & 15u;
    // (uniform per wavefront) every line in front of consumed_end ends in a newline: i < n_nl
    for (uint32_t i0 = (tid >> 6) * 4u; i0 < n_nl; i0 += (n_thr >> 6) * 4u) {
        const uint32_t i = i0 + sub;
        uint32_t b = 0, len = 0, d = 0;
        if (i < n_nl) {
            b = i ? nlpos[i - 1] + 1 : start;
            if (b < stop) {
                const uint32_t e = nlpos[i], c = b < e ? raw[b] : '\n';
                if (c != '>' && c != '@' && c != '+' && c != '\n') {
                    len = e - b;
                    d = dest[i];
                }
            }
        }
        if (len && len < FA_LONG) fa_copy<4u>(raw, b, len, packed + d, l16, 16u);
        if (__any(len >= FA_LONG)) {
#pragma unroll
            for (uint32_t q = 0; q < 4; ++q) {
                const uint32_t qb = __shfl(b, q * 16), ql = __shfl(len, q * 16), qd = __shfl(d, q * 16);
                if (ql >= FA_LONG) fa_copy<16u>(raw, qb, ql, packed + qd, lane, 64u);
            }
        }
        if (__builtin_amdgcn_readfirstlane(b) >= stop) break;     // (uniform; lines are in file order: nothing further lies in front of stop)
    }
}

// ---- subsampling: A4, A7 and A8 again, off the default path ---------------------------------------------------------------------
// A4 in three phases.  0: header lines per block -> bsum_hdr (A5 scans it).  1 and 2: the header lines in front of line i give its
// record's number, the rule says whether that record is kept, and the scanned value is A4's with the bytes of a dropped record's lines
// and the 1 of its header line (the record's '\n') left out: block sums -> bsum (A5 again), then everything A4 writes.  dest of a
// line that is not copied is FA_NONE; rec_d[r + 1] == rec_d[r] says that record r was dropped.
__global__ __launch_bounds__(1024) void fa_lines_sub_kernel(const uint8_t* raw, FqState* st, const uint32_t* nlpos, uint32_t tail_max, uint32_t n_new,
                                                            const uint32_t* n_new_dev, unsigned long long* bsum_hdr, unsigned long long* bsum,
                                                            uint32_t* dest, uint32_t* rec_d, uint32_t* rec_pos, int phase, uint32_t cap_lines,
                                                            unsigned long long seed, unsigned long long threshold)
{
    __shared__ unsigned long long sh[16];
    if (fa_skip(st, cap_lines)) return;
    const uint32_t end = fa_end(tail_max, n_new, n_new_dev);
    const uint32_t L = fa_n_lines(st, nlpos, end);
    if (blockIdx.x * 1024u >= L) return;      // (uniform) the launch is sized for the arrays' capacity
    const uint32_t i = blockIdx.x * 1024u + threadIdx.x;
    uint32_t s = 0, c = '\n', len = 0;
    bool hdr = false;
    if (i < L) {
        s = i ? nlpos[i - 1] + 1 : st->start;
        const uint32_t e = i < st->n_lines ? nlpos[i] : end;
        if (s < e) c = raw[s];
        hdr = c == '>' || c == '@';
        if (!hdr && c != '+' && c != '\n') len = e - s;
    }
    unsigned long long tot;
    const unsigned long long exh = fa_block_scan_excl(hdr ? 1ull << 32 : 0ull, sh, &tot);
    if (phase == 0) {
        if (threadIdx.x == 0) bsum_hdr[blockIdx.x] = tot;
        return;
    }
    const uint32_t n_hdr = (uint32_t)((bsum_hdr[blockIdx.x] + exh) >> 32);      // header lines in front of line i
    bool keep = false;
    if (hdr || len) keep = vgh::subsample_keep(st->n_seen + (hdr ? n_hdr : n_hdr ? n_hdr - 1u : 0u), seed, threshold);
    const unsigned long long v = hdr ? (1ull << 32) | (keep ? 1u : 0u) : keep ? len : 0u;
    const unsigned long long ex = fa_block_scan_excl(v, sh, &tot);
    if (phase == 1) {
        if (threadIdx.x == 0) bsum[blockIdx.x] = tot;
        return;
    }
    if (i >= L) return;
    const unsigned long long e = bsum[blockIdx.x] + ex;
    const uint32_t hi = (uint32_t)(e >> 32), lo = (uint32_t)e;
    dest[i] = keep && len ? lo - 1u : FA_NONE;      // (a kept sequence line follows its record's header line: lo >= 1)
    if (hdr) {
        if (hi < fasta_cap_rec(cap_lines)) {
            rec_d[hi] = lo;
            rec_pos[hi] = s;
        }
    } else if (c == '+' && hi) {
        atomicMin(&st->first_bad, hi - 1u);
    }
}

// A7: one workgroup counts the kept records among the accepted ones (rec_d moves on over a kept record: by its '\n' at least), then
// thread 0 does A7's bookkeeping and moves n_seen on by every accepted record
__global__ __launch_bounds__(1024) void fa_finish_sub_kernel(const uint8_t* raw, FqState* st, const unsigned long long* total, const uint32_t* rec_d,
                                                            const uint32_t* rec_pos, uint32_t n_new, const uint32_t* n_new_dev, uint32_t cap_lines,
                                                            uint32_t tail_max)
{
    __shared__ uint32_t sh[16];
    const uint32_t end = fa_end(tail_max, n_new, n_new_dev);
    const bool live = !st->stopped && st->start < end;
    const uint32_t first_bad = st->first_bad;
    bool unfit = false;
    uint32_t good = 0, H = 0;
    if (live) {
        const uint32_t c0 = raw[st->start];
        unfit = st->dirty || st->n_lines > cap_lines || (c0 != '>' && c0 != '@');
        if (!unfit) {
            H = (uint32_t)(*total >> 32);     // >= 1: line 0 is a header line; record H - 1 is the one carried
            good = first_bad < H - 1u ? first_bad : H - 1u;
        }
    }
    uint32_t mine = 0;
    for (uint32_t r = threadIdx.x; r < good; r += blockDim.x) mine += rec_d[r + 1] > rec_d[r];
    const uint32_t kept = block_reduce_add(mine, sh);      // (its barriers: every thread has read the state before thread 0 writes it)
    if (threadIdx.x) return;
    uint32_t consumed_end = st->start, packed = 0;
    if (live) {
        if (unfit) {
            st->stopped = 1;     // nothing of this chunk is taken: the host reader resumes at its first byte
        } else {
            if (first_bad < H) st->stopped = 1;
            consumed_end = rec_pos[good];
            packed = rec_d[good];
        }
    }
    st->n_good = good;
    st->packed_bytes = packed;
    st->n_seen += good;
    st->n_records += kept;
    st->n_bases += packed - kept;
    st->consumed += consumed_end - st->start;
    st->consumed_end = consumed_end;
    uint32_t tail = st->stopped ? 0u : end - consumed_end;
    if (tail > tail_max) {      // a record longer than the carry buffer (a contig, not a read): the host reader's
        st->stopped = 1;
        tail = 0;
    }
    st->tail_len = tail;
}

// A8: the '\n' behind every kept accepted record, and the lines that have a place in the block (dest != FA_NONE)
__global__ __launch_bounds__(256) void fa_pack_sub_kernel(const uint8_t* raw, const FqState* st, const uint32_t* nlpos, const uint32_t* dest,
                                                          const uint32_t* rec_d, uint8_t* packed)
{
    const uint32_t good = st->n_good;
    if (!good) return;
    const uint32_t stop = st->consumed_end, start = st->start, n_nl = st->n_lines;
    const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x, n_thr = gridDim.x * blockDim.x;
    for (uint32_t r = tid + 1; r <= good; r += n_thr)
        if (rec_d[r] > rec_d[r - 1]) packed[rec_d[r] - 1u] = '\n';
    const uint32_t lane = threadIdx.x & 63u, sub = lane >> 4, l16 = lane & 15u;
    for (uint32_t i0 = (tid >> 6) * 4u; i0 < n_nl; i0 += (n_thr >> 6) * 4u) {
        const uint32_t i = i0 + sub;
        uint32_t b = 0, len = 0, d = 0;
        if (i < n_nl) {
            b = i ? nlpos[i - 1] + 1 : start;
            if (b < stop) {
                const uint32_t e = nlpos[i], c = b < e ? raw[b] : '\n';
                if (c != '>' && c != '@' && c != '+' && c != '\n' && dest[i] != FA_NONE) {
                    len = e - b;
                    d = dest[i];
                }
            }
        }
        if (len && len < FA_LONG) fa_copy<4u>(raw, b, len, packed + d, l16, 16u);
        if (__any(len >= FA_LONG)) {
#pragma unroll
            for (uint32_t q = 0; q < 4; ++q) {
                const uint32_t qb = __shfl(b, q * 16), ql = __shfl(len, q * 16), qd = __shfl(d, q * 16);
                if (ql >= FA_LONG) fa_copy<16u>(raw, qb, ql, packed + qd, lane, 64u);
            }
        }
        if (__builtin_amdgcn_readfirstlane(b) >= stop) break;     // (uniform; lines are in file order: nothing further lies in front of stop)
    }
}

// A9: the unconsumed tail goes in front of the next chunk's landing area, and the per-chunk state is re-armed
__global__ __launch_bounds__(1024) void fa_carry_kernel(const uint8_t* raw, uint8_t* raw_next, FqState* st, uint32_t tail_max)
{
    const uint32_t tail = st->tail_len, from = st->consumed_end;
    fa_copy<16u>(raw, from, tail, raw_next + (tail_max - tail), threadIdx.x, blockDim.x);
    __syncthreads();
    if (threadIdx.x == 0) {
        st->start = tail_max - tail;
        st->first_bad = FA_NONE;
        st->dirty = 0;
        st->n_lines = 0;
    }
}

// ---- launcher: everything one chunk needs, in stream order --------------------------------------------------------------------
hipError_t launch_fasta_chunk(const FaBuffers& b, uint32_t n_new, hipStream_t s, const uint32_t* n_new_dev)
{
    const FqBuffers& q = b.q;
    hipError_t e = launch_fastq_lines(q, n_new, s, n_new_dev);      // A1-A3: st->n_lines, st->dirty, nlpos
    if (e != hipSuccess) return e;
    const uint32_t n_lblk = q.cap_lines / 1024u + 1;      // cap_lines + 1 lines at most
    const uint32_t cap_rec = fasta_cap_rec(q.cap_lines);
    const uint32_t rgrid = (cap_rec + 255u) / 256u < 2048u ? (cap_rec + 255u) / 256u : 2048u;
    if (q.sub.on) {
        for (int phase = 0; phase < 3; ++phase) {
            hipLaunchKernelGGL(fa_lines_sub_kernel, dim3(n_lblk), dim3(1024), 0, s, q.raw, q.state, q.nlpos, q.tail_max, n_new, n_new_dev, b.bsum_hdr,
                               b.bsum, b.dest, b.rec_d, b.rec_pos, phase, q.cap_lines, q.sub.seed, q.sub.threshold);
            if (phase < 2)
                hipLaunchKernelGGL(fa_scan_sums_kernel, dim3(1), dim3(1024), 0, s, q.state, q.nlpos, q.tail_max, n_new, n_new_dev,
                                   phase ? b.bsum : b.bsum_hdr, b.total, q.cap_lines);
        }
        hipLaunchKernelGGL(fa_records_kernel, dim3(rgrid), dim3(256), 0, s, q.state, b.total, b.rec_d, b.rec_pos, q.cap_lines, q.tail_max);
        hipLaunchKernelGGL(fa_finish_sub_kernel, dim3(1), dim3(1024), 0, s, q.raw, q.state, b.total, b.rec_d, b.rec_pos, n_new, n_new_dev, q.cap_lines,
                           q.tail_max);
        hipLaunchKernelGGL(fa_pack_sub_kernel, dim3(2048), dim3(256), 0, s, q.raw, q.state, q.nlpos, b.dest, b.rec_d, q.packed);
        hipLaunchKernelGGL(fa_carry_kernel, dim3(1), dim3(1024), 0, s, q.raw, q.raw_next, q.state, q.tail_max);
        return hipGetLastError();
    }
    hipLaunchKernelGGL(fa_lines_kernel, dim3(n_lblk), dim3(1024), 0, s, q.raw, q.state, q.nlpos, q.tail_max, n_new, n_new_dev, b.bsum, b.dest, b.rec_d,
                       b.rec_pos, 0, q.cap_lines);
    hipLaunchKernelGGL(fa_scan_sums_kernel, dim3(1), dim3(1024), 0, s, q.state, q.nlpos, q.tail_max, n_new, n_new_dev, b.bsum, b.total, q.cap_lines);
    hipLaunchKernelGGL(fa_lines_kernel, dim3(n_lblk), dim3(1024), 0, s, q.raw, q.state, q.nlpos, q.tail_max, n_new, n_new_dev, b.bsum, b.dest, b.rec_d,
                       b.rec_pos, 1, q.cap_lines);
    hipLaunchKernelGGL(fa_records_kernel, dim3(rgrid), dim3(256), 0, s, q.state, b.total, b.rec_d, b.rec_pos, q.cap_lines, q.tail_max);
    hipLaunchKernelGGL(fa_finish_kernel, dim3(1), dim3(1), 0, s, q.raw, q.state, b.total, b.rec_d, b.rec_pos, n_new, n_new_dev, q.cap_lines, q.tail_max);
    hipLaunchKernelGGL(fa_pack_kernel, dim3(2048), dim3(256), 0, s, q.raw, q.state, q.nlpos, b.dest, b.rec_d, q.packed);
    hipLaunchKernelGGL(fa_carry_kernel, dim3(1), dim3(1024), 0, s, q.raw, q.raw_next, q.state, q.tail_max);
    return hipGetLastError();
}

}  // namespace vgk
