// vgmi_bam.hip -- BAM records on the device (gfx950): the reads of a BAM / unaligned BAM file, taken from the text the block-gzip
// inflate kernel (vgmi_inflate.hip) has just written, into the same '\n'-joined read block the FASTQ parser writes.
//
// Which records are reads, and what a read is (the records `samtools fastq` writes by default; SAM spec 4.2):
//   kept      flag & 0x900 == 0 (no secondary, no supplementary alignment) and l_seq > 0 (SEQ '*' has no bases: the
//             reference aborts on an empty read, kmer.cpp:124)
//   sequence  the l_seq bases of the 4-bit SEQ field, high nibble first, through "=ACMGRSVTWYHKDBN", as stored (a
//             reverse-strand record adds the same canonical k-mers as its reverse complement)
// A record is valid when its block_size stays inside the data, l_read_name >= 1 and the name's last byte is NUL,
// 32 + l_read_name + 4 n_cigar_op + ceil(l_seq / 2) + l_seq <= block_size, and refID, next_refID lie in [-1, n_ref).
// The first record that is not valid -- or is longer than the 1 MiB carry between chunks, wherever it lies -- stops the device for good, and the
// host decoder (csrc/host/bam_reader.cpp, which names the fault) takes the stream over at that record's first byte.
//
// Records are a chain of length prefixes (next = off + 4 + block_size) that need not line up with anything else, and a serial
// walk is one dependent load per record.  So, per chunk, all on one HIP stream:
//   B0 the header bytes still to pass over ->
//   B1 candidate test at every byte offset (all the checks above: they are local to the record) -> B2 scan of the per-tile
//   counts -> B3 candidate offsets, in order ->
//   B4 successor of every candidate (the candidate at off + 4 + block_size, or the terminal) ->
//   B5 the chain from the chunk's first byte (a record boundary: the carried record, or the first byte behind the header):
//   rounds of pointer doubling, round r marks the successors at distance 2^r of everything marked and squares the jump ->
//   B6 l_seq + 1 of every kept record of the chain, B7 scan -> B8 4-bit decode, a wavefront per record ->
//   B9 bookkeeping (records, bases, consumed bytes, tail; where the chain ends) -> B10 tail carried into the other raw buffer.
// Offsets are absolute in the raw buffer (tail_max bytes of carry area, then the chunk), so they fit 32 bits.
// With subsampling (BamBuffers::sub; vgmi_fastq_set_subsample) a read's number in the file is FqState::n_seen + its rank among the
// chain's reads: between B6 and B7, bam_rank_kernel scans the reads (B7's two phases) and turns rec_bytes of those the rule drops
// to 0, which B7 and B8 pass over as they pass over the records the filter drops; B9 is bam_finish_sub_kernel.
// With a configured read filter (BamBuffers::filt; vgmi_fastq_set_bam_filter, the rule in vgmi_bam_filter.h) B6 is
// bam_keep_filter_kernel, with a tag bound bam_cut_kernel ends the chain in front of a record whose auxiliary fields cannot be walked,
// and B9 is bam_finish_filter_kernel / bam_finish_filter_sub_kernel; the kernels between run on the rec_bytes these leave.
// With a region list (BamBuffers::regions; vgmi_fastq_set_bam_regions) B6 is bam_keep_region_kernel, the filter's B6 with the region test
// in front of the tag walk; bam_cut_kernel and B9 as with a filter.
// With a read filter (BamBuffers::rf; vgmi_fastq_set_read_filter, the rule in vgmi_read_filter.h) bam_read_filter_kernel runs in front of
// B7 on the rec_bytes all of the above leave, and B9 is bam_finish_rf_kernel.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vgmi_bam_filter.h"
#include "vgmi_read_filter.h"
#include "vgmi_subsample.h"
#include "vgmi_block_scan.h"
#include "vgmi_kernels.h"

namespace vgk {

#define BAM_PIECES 4u                      // 16-byte pieces per thread in the byte-parallel kernels, 4 KiB apart (as vgmi_fastq.hip)
#define BAM_TILE (4096u * BAM_PIECES)
#define BAM_NONE 0xFFFFFFFFu
#define BAM_GRID 2048u                     // workgroups of the candidate-parallel kernels (grid-stride)

__device__ __forceinline__ uint32_t bam_end(uint32_t tail_max, uint32_t n_new, const uint32_t* n_new_dev)
{
    if (n_new_dev) {
        const uint32_t d = *n_new_dev;
        n_new = d < n_new ? d : n_new;
    }
    return tail_max + n_new;
}

// the little-endian dword at byte o of raw: two aligned loads (the raw buffer has slack behind the data) and a funnel shift
__device__ __forceinline__ uint32_t bam_ld32(const uint8_t* raw, uint32_t o)
{
    const uint32_t* w = reinterpret_cast<const uint32_t*>(raw + (o & ~3u));
    return __builtin_amdgcn_alignbyte(w[1], w[0], o & 3u);
}

// the checks of the header comment on the fixed part of a record at o: 0 whole and valid so far (the name's NUL is the caller's),
// 1 the data ends inside the record or its block_size, 2 whole but not a valid record
__device__ __forceinline__ int bam_fixed(uint32_t o, uint32_t end, uint32_t bs, uint32_t ref, uint32_t l_rn, uint32_t n_cig, uint32_t l_seq,
                                         uint32_t next_ref, int32_t n_ref)
{
    if (end - o < 4u || (unsigned long long)o + 4u + bs > end) return 1;
    const bool ok = bs >= 32u && (int32_t)ref >= -1 && (int32_t)ref < n_ref && (int32_t)next_ref >= -1 && (int32_t)next_ref < n_ref &&
                    l_rn >= 1u && 32ull + l_rn + 4ull * n_cig + (l_seq + 1ull) / 2u + l_seq <= bs;
    return ok ? 0 : 2;
}

// the same from global memory (one thread): o < end
__device__ int bam_check(const uint8_t* raw, uint32_t o, uint32_t end, int32_t n_ref, uint32_t* block_size)
{
    if (end - o < 4u) return 1;
    const uint32_t bs = bam_ld32(raw, o);
    *block_size = bs;
    if ((unsigned long long)o + 4u + bs > end) return 1;
    if (bs < 32u) return 2;
    const uint32_t w16 = bam_ld32(raw, o + 16);
    const uint32_t l_rn = raw[o + 12];
    const int r = bam_fixed(o, end, bs, bam_ld32(raw, o + 4), l_rn, w16 & 0xFFFFu, bam_ld32(raw, o + 20), bam_ld32(raw, o + 24), n_ref);
    if (r) return r;
    return raw[o + 36 + l_rn - 1] == 0 ? 0 : 2;
}

// bit jj of the result: a whole, valid record no longer than the carry starts at off + jj (off 16-aligned, lo <= off + jj < end)
__device__ __forceinline__ uint32_t bam_cand_mask(const uint8_t* raw, uint32_t off, uint32_t lo, uint32_t end, int32_t n_ref, uint32_t tail_max)
{
    uint32_t w[17];   // bytes off .. off + 63 (zeros behind the data) and a pad dword for the funnel shift
#pragma unroll
    for (uint32_t q = 0; q < 4; ++q) {
        const uint4 v = off + 16u * q < end ? *reinterpret_cast<const uint4*>(raw + off + 16u * q) : make_uint4(0u, 0u, 0u, 0u);
        w[4 * q] = v.x;
        w[4 * q + 1] = v.y;
        w[4 * q + 2] = v.z;
        w[4 * q + 3] = v.w;
    }
    w[16] = 0;
    uint32_t m = 0;
#pragma unroll
    for (uint32_t jj = 0; jj < 16; ++jj) {
        const uint32_t o = off + jj;
#define BAM_W(b) __builtin_amdgcn_alignbyte(w[((b) >> 2) + 1], w[(b) >> 2], (b) & 3u)
        const uint32_t bs = BAM_W(jj), ref = BAM_W(jj + 4), w12 = BAM_W(jj + 12), w16 = BAM_W(jj + 16), l_seq = BAM_W(jj + 20),
                       next_ref = BAM_W(jj + 24);
#undef BAM_W
        if (o >= lo && o < end && bs <= tail_max - 4u && bam_fixed(o, end, bs, ref, w12 & 0xFFu, w16 & 0xFFFFu, l_seq, next_ref, n_ref) == 0 &&
            raw[o + 36 + (w12 & 0xFFu) - 1] == 0)
            m |= 1u << jj;
    }
    return m;
}

// B0: the header (magic .. the last reference) is passed over, however many chunks it spans
__global__ void bam_begin_kernel(FqState* st, BamState* bs, uint32_t tail_max, uint32_t n_new, const uint32_t* n_new_dev)
{
    if (threadIdx.x || blockIdx.x || st->stopped || !bs->hdr_left) return;
    const uint32_t end = bam_end(tail_max, n_new, n_new_dev);
    const unsigned long long avail = end - st->start;
    const uint32_t skip = (uint32_t)(bs->hdr_left < avail ? bs->hdr_left : avail);
    st->start += skip;
    st->consumed += skip;
    bs->hdr_left -= skip;
}

// B1: candidates per tile
__global__ __launch_bounds__(256) void bam_count_kernel(const uint8_t* raw, const FqState* st, uint32_t tail_max, uint32_t n_new,
                                                        const uint32_t* n_new_dev, int32_t n_ref, uint32_t* tile_cnt)
{
    __shared__ uint32_t sh[4];
    const uint32_t end = bam_end(tail_max, n_new, n_new_dev);
    const uint32_t start = st->start, off0 = blockIdx.x * BAM_TILE + threadIdx.x * 16u;
    uint32_t n = 0;
    if (!st->stopped) {
#pragma unroll
        for (uint32_t j = 0; j < BAM_PIECES; ++j) {
            const uint32_t off = off0 + j * 4096u;
            if (off < end && off + 16 > start) n += __popc(bam_cand_mask(raw, off, start, end, n_ref, tail_max));
        }
    }
    const uint32_t t = block_reduce_add(n, sh);
    if (threadIdx.x == 0) tile_cnt[blockIdx.x] = t;
}

// B3: candidate offsets in order (tile_base: B2's scan of B1's counts; its total is bs->n_cand)
__global__ __launch_bounds__(256) void bam_cand_kernel(const uint8_t* raw, const FqState* st, const BamState* bs, uint32_t tail_max, uint32_t n_new,
                                                       const uint32_t* n_new_dev, int32_t n_ref, const uint32_t* tile_base, uint32_t* cand,
                                                       uint32_t cap)
{
    __shared__ uint32_t sh[4];
    if (st->stopped || bs->n_cand > cap) return;   // (uniform) too many: nothing of this chunk is taken
    const uint32_t end = bam_end(tail_max, n_new, n_new_dev);
    const uint32_t start = st->start, off0 = blockIdx.x * BAM_TILE + threadIdx.x * 16u;
    uint32_t base = tile_base[blockIdx.x];
#pragma unroll
    for (uint32_t j = 0; j < BAM_PIECES; ++j) {
        const uint32_t off = off0 + j * 4096u;
        uint32_t m = off < end && off + 16 > start ? bam_cand_mask(raw, off, start, end, n_ref, tail_max) : 0u;
        uint32_t tot;
        uint32_t pos = base + block_scan_excl(__popc(m), sh, &tot);
        base += tot;
        while (m) {
            const uint32_t q = __builtin_ctz(m);
            m &= m - 1;
            cand[pos++] = off + q;
        }
    }
}

// B4: successor of every candidate; the terminal (index n) stands for "no candidate there" and leads to itself
__global__ __launch_bounds__(256) void bam_link_kernel(const uint8_t* raw, const FqState* st, const BamState* bs, const uint32_t* cand,
                                                       uint32_t* j0, uint8_t* mark, uint32_t cap)
{
    const uint32_t n = bs->n_cand;
    if (n > cap) return;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i <= n; i += gridDim.x * blockDim.x) {
        if (i == n) {
            j0[n] = n;
            mark[n] = 0;
            continue;
        }
        const uint32_t o = cand[i];
        const uint32_t nx = o + 4u + bam_ld32(raw, o);
        // mostly the next candidate or one of the few behind it (a false candidate is rare); else a binary search
        uint32_t lo = i + 1, hi = n, j = n;
        for (uint32_t t = 0; t < 4 && lo < hi; ++t, ++lo) {
            const uint32_t c = cand[lo];
            if (c >= nx) {
                hi = lo;
                if (c == nx) j = lo;
                break;
            }
        }
        while (j == n && lo < hi) {
            const uint32_t mid = lo + (hi - lo) / 2, c = cand[mid];
            if (c == nx) j = mid;
            else if (c < nx) lo = mid + 1;
            else hi = mid;
        }
        j0[i] = j;
        mark[i] = i == 0 && o == st->start;
    }
}

// B5 round r: everything marked marks its successor at distance 2^r (J = src), and dst = J o J.  After round r the nodes at
// distance 0 .. 2^(r+1) - 1 from the start are marked; a node marked early in the same round only marks further chain nodes.
__global__ __launch_bounds__(256) void bam_jump_kernel(const BamState* bs, const uint32_t* src, uint32_t* dst, uint8_t* mark, uint32_t r,
                                                       uint32_t cap)
{
    const uint32_t n = bs->n_cand;
    if (n > cap || (1ull << r) >= n) return;   // (uniform) the chain is at most n long
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i <= n; i += gridDim.x * blockDim.x) {
        const uint32_t t = src[i];
        dst[i] = src[t];
        if (mark[i]) mark[t] = 1;
    }
}

// B6: packed bytes of every kept record of the chain; the chain's last record (successor: the terminal)
__global__ __launch_bounds__(256) void bam_keep_kernel(const uint8_t* raw, BamState* bs, const uint32_t* cand, const uint32_t* j0, const uint8_t* mark,
                                                       uint32_t* rec_bytes, uint32_t cap)
{
    __shared__ uint32_t sh[4];
    const uint32_t n = bs->n_cand;
    if (n > cap) return;
    uint32_t kept = 0;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        uint32_t b = 0;
        if (mark[i]) {
            const uint32_t o = cand[i];
            const uint32_t flag = bam_ld32(raw, o + 16) >> 16, l_seq = bam_ld32(raw, o + 20);
            if (!(flag & 0x900u) && l_seq) {
                b = l_seq + 1;
                ++kept;
            }
            if (j0[i] == n) bs->last = i;
        }
        rec_bytes[i] = b;
    }
    const uint32_t t = block_reduce_add(kept, sh);
    if (threadIdx.x == 0 && t) atomicAdd(&bs->n_kept, t);
}

// B7: scan of rec_bytes: block sums (phase 0), then (after launch_scan_small over the sums) the offsets (phase 1)
__global__ __launch_bounds__(1024) void bam_scan_blocks_kernel(const uint32_t* v, const BamState* bs, uint32_t* block_sum, uint32_t* out, int phase,
                                                              uint32_t cap)
{
    __shared__ uint32_t sh[16];
    const uint32_t n = bs->n_cand;
    if (n > cap) return;
    if (blockIdx.x * 1024u >= n) {      // (uniform) the launch is sized for the capacity
        if (phase == 0 && threadIdx.x == 0) block_sum[blockIdx.x] = 0;
        return;
    }
    const uint32_t i = blockIdx.x * 1024u + threadIdx.x;
    uint32_t tot;
    const uint32_t ex = block_scan_excl(i < n ? v[i] : 0u, sh, &tot);
    if (phase == 0) {
        if (threadIdx.x == 0) block_sum[blockIdx.x] = tot;
    } else if (i < n) {
        out[i] = block_sum[blockIdx.x] + ex;
    }
}

// B8: 4-bit SEQ -> ASCII, a wavefront per kept record, two bases per lane and byte
__global__ __launch_bounds__(256) void bam_decode_kernel(const uint8_t* raw, const BamState* bs, const uint32_t* cand, const uint32_t* rec_bytes,
                                                         const uint32_t* out_off, uint8_t* packed, uint32_t cap)
{
    const uint32_t n = bs->n_cand;
    if (n > cap) return;
    const char* nt16 = "=ACMGRSVTWYHKDBN";
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = (gridDim.x * blockDim.x) >> 6;
    for (uint32_t i = wave; i < n; i += n_waves) {
        const uint32_t nb = rec_bytes[i];
        if (!nb) continue;
        const uint32_t o = cand[i], l_seq = nb - 1;
        const uint32_t s = o + 36u + raw[o + 12] + 4u * (bam_ld32(raw, o + 16) & 0xFFFFu);
        uint8_t* dst = packed + out_off[i];
        for (uint32_t k = lane; 2 * k < l_seq; k += 64) {
            const uint32_t b = raw[s + k];
            dst[2 * k] = nt16[b >> 4];
            if (2 * k + 1 < l_seq) dst[2 * k + 1] = nt16[b & 15u];
        }
        if (lane == 0) dst[l_seq] = '\n';
    }
}

// B8 with a minimum base quality: the same decode, and the lane that decodes byte k of SEQ loads QUAL[2k] and QUAL[2k + 1] -- QUAL
// lies (l_seq + 1) / 2 bytes behind SEQ inside the record (the candidate test has checked that it fits), base i pairs with QUAL[i] in
// record order whatever the strand flag says.  A base whose QUAL is below `bound` is decoded as 'N'; a record whose QUAL[0] is 0xff
// stores no qualities and is decoded as it is.  Records the filter drops (rec_bytes == 0) are not looked at.  The masked bases are
// summed over the workgroup and added to FqState::n_masked once.
__global__ __launch_bounds__(256) void bam_decode_mask_kernel(const uint8_t* raw, FqState* st, const BamState* bs, const uint32_t* cand,
                                                              const uint32_t* rec_bytes, const uint32_t* out_off, uint8_t* packed, uint32_t cap,
                                                              uint32_t bound)
{
    __shared__ uint32_t sh[4];
    const uint32_t n = bs->n_cand;
    if (n > cap) return;   // (uniform)
    const char* nt16 = "=ACMGRSVTWYHKDBN";
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = (gridDim.x * blockDim.x) >> 6;
    uint32_t masked = 0;
    for (uint32_t i = wave; i < n; i += n_waves) {
        const uint32_t nb = rec_bytes[i];
        if (!nb) continue;
        const uint32_t o = cand[i], l_seq = nb - 1;
        const uint32_t s = o + 36u + raw[o + 12] + 4u * (bam_ld32(raw, o + 16) & 0xFFFFu);
        const uint32_t q = s + (l_seq + 1u) / 2u;
        const uint32_t lim = raw[q] == 0xFFu ? 0u : bound;   // (uniform over the wavefront)
        uint8_t* dst = packed + out_off[i];
        for (uint32_t k = lane; 2 * k < l_seq; k += 64) {
            const uint32_t b = raw[s + k];
            const bool low0 = raw[q + 2 * k] < lim;
            dst[2 * k] = low0 ? 'N' : nt16[b >> 4];
            masked += low0;
            if (2 * k + 1 < l_seq) {
                const bool low1 = raw[q + 2 * k + 1] < lim;
                dst[2 * k + 1] = low1 ? 'N' : nt16[b & 15u];
                masked += low1;
            }
        }
        if (lane == 0) dst[l_seq] = '\n';
    }
    const uint32_t t = block_reduce_add(masked, sh);
    if (threadIdx.x == 0 && t) atomicAdd(&st->n_masked, (unsigned long long)t);
}

// B9: chunk bookkeeping (one thread)
__global__ void bam_finish_kernel(const uint8_t* raw, FqState* st, const BamState* bs, const uint32_t* cand, const uint32_t* rec_bytes,
                                  const uint32_t* out_off, uint32_t n_new, const uint32_t* n_new_dev, uint32_t cap, uint32_t tail_max, int32_t n_ref)
{
    if (threadIdx.x || blockIdx.x) return;
    const uint32_t end = bam_end(tail_max, n_new, n_new_dev);
    uint32_t kept = 0, packed = 0, chain_end = st->start, tail = 0;
    if (!st->stopped) {
        const uint32_t n = bs->n_cand;
        if (n > cap) {
            st->stopped = 1;     // more candidates than the arrays hold: nothing of this chunk is taken, the host resumes at its first byte
        } else {
            if (bs->last != BAM_NONE) {
                const uint32_t o = cand[bs->last];
                chain_end = o + 4u + bam_ld32(raw, o);
                kept = bs->n_kept;
                packed = out_off[n - 1] + rec_bytes[n - 1];
            }
            if (chain_end < end) {
                // what follows the chain: the front of a record the next chunk completes, or something the host must judge
                uint32_t block_size = 0;
                const int r = bam_check(raw, chain_end, end, n_ref, &block_size);
                if (r == 1 && (end - chain_end < 4u || block_size <= tail_max - 4u)) tail = end - chain_end;
                else st->stopped = 1;     // not a valid record, or one longer than the carry (whole or not: never a candidate)
            }
        }
    }
    st->n_good = kept;
    st->packed_bytes = packed;
    st->n_records += kept;
    st->n_bases += packed - kept;
    st->consumed += chain_end - st->start;
    st->consumed_end = chain_end;
    st->tail_len = tail;
}

// ---- subsampling, off the default path ------------------------------------------------------------------------------------------
// Between B6 and B7: the rank of every read among the chain's reads -- block sums (phase 0), then (after launch_scan_small over
// the sums) the ranks; read number n_seen + rank of the file is kept or its rec_bytes turned to 0.  The reads dropped are added up
// in BamState::n_dropped: n_kept stays the chain's reads.
__global__ __launch_bounds__(1024) void bam_rank_kernel(uint32_t* rec_bytes, const FqState* st, BamState* bs, uint32_t* block_sum, int phase,
                                                       uint32_t cap, unsigned long long seed, unsigned long long threshold)
{
    __shared__ uint32_t sh[16];
    const uint32_t n = bs->n_cand;
    if (n > cap) return;
    if (blockIdx.x * 1024u >= n) {      // (uniform) the launch is sized for the capacity
        if (phase == 0 && threadIdx.x == 0) block_sum[blockIdx.x] = 0;
        return;
    }
    const uint32_t i = blockIdx.x * 1024u + threadIdx.x;
    const bool read = i < n && rec_bytes[i] != 0u;
    uint32_t tot;
    const uint32_t ex = block_scan_excl(read ? 1u : 0u, sh, &tot);
    if (phase == 0) {
        if (threadIdx.x == 0) block_sum[blockIdx.x] = tot;
        return;
    }
    const bool drop = read && !vgh::subsample_keep(st->n_seen + block_sum[blockIdx.x] + ex, seed, threshold);
    if (drop) rec_bytes[i] = 0;
    const uint32_t d = block_reduce_add(drop ? 1u : 0u, sh);
    if (threadIdx.x == 0 && d) atomicAdd(&bs->n_dropped, d);
}

// B9: the chain's reads move n_seen on, the kept ones are the chunk's records
__global__ void bam_finish_sub_kernel(const uint8_t* raw, FqState* st, BamState* bs, const uint32_t* cand, const uint32_t* rec_bytes,
                                      const uint32_t* out_off, uint32_t n_new, const uint32_t* n_new_dev, uint32_t cap, uint32_t tail_max,
                                      int32_t n_ref)
{
    if (threadIdx.x || blockIdx.x) return;
    const uint32_t end = bam_end(tail_max, n_new, n_new_dev);
    uint32_t reads = 0, kept = 0, packed = 0, chain_end = st->start, tail = 0;
    if (!st->stopped) {
        const uint32_t n = bs->n_cand;
        if (n > cap) {
            st->stopped = 1;     // more candidates than the arrays hold: nothing of this chunk is taken, the host resumes at its first byte
        } else {
            if (bs->last != BAM_NONE) {
                const uint32_t o = cand[bs->last];
                chain_end = o + 4u + bam_ld32(raw, o);
                reads = bs->n_kept;
                kept = reads - bs->n_dropped;
                packed = out_off[n - 1] + rec_bytes[n - 1];
            }
            if (chain_end < end) {
                // what follows the chain: the front of a record the next chunk completes, or something the host must judge
                uint32_t block_size = 0;
                const int r = bam_check(raw, chain_end, end, n_ref, &block_size);
                if (r == 1 && (end - chain_end < 4u || block_size <= tail_max - 4u)) tail = end - chain_end;
                else st->stopped = 1;     // not a valid record, or one longer than the carry (whole or not: never a candidate)
            }
        }
    }
    bs->n_dropped = 0;
    st->n_good = kept;
    st->packed_bytes = packed;
    st->n_seen += reads;
    st->n_records += kept;
    st->n_bases += packed - kept;
    st->consumed += chain_end - st->start;
    st->consumed_end = chain_end;
    st->tail_len = tail;
}

// ---- the configured read filter, off the default path ------------------------------------------------------------------------------
// a record's bytes for the rule of vgmi_bam_filter.h: offsets in the raw buffer, dwords by two aligned loads and a funnel shift, the
// NUL of a Z / H value by aligned dwords (the bytes in front of p are made non-zero; the lowest flagged byte of the zero-byte test
// is exact).  Every load lies below `end` rounded up to a dword plus one dword: inside the raw buffer's slack.
struct BamBytes {
    const uint8_t* raw;
    __device__ __forceinline__ uint32_t u8(uint32_t p) const { return raw[p]; }
    __device__ __forceinline__ uint32_t u32(uint32_t p) const { return bam_ld32(raw, p); }
    __device__ __forceinline__ uint32_t find_nul(uint32_t p, uint32_t end) const
    {
        uint32_t a = p & ~3u;
        uint32_t w = *reinterpret_cast<const uint32_t*>(raw + a) | ((1u << (8u * (p & 3u))) - 1u);
        for (;;) {
            const uint32_t z = (w - 0x01010101u) & ~w & 0x80808080u;
            if (z) {
                const uint32_t q = a + ((uint32_t)__builtin_ctz(z) >> 3);
                return q < end ? q : end;
            }
            a += 4u;
            if (a >= end) return end;
            w = *reinterpret_cast<const uint32_t*>(raw + a);
        }
    }
};

// B6 with a filter set: rec_bytes by bam_filter_verdict, a lane per chain record -- the fixed fields decide most records, a B array is
// passed over by arithmetic and only a Z / H value is scanned, a dword a step, so a wavefront per record would idle 63 lanes on
// all but the longest strings.  The chain's records and the reads among them are summed per workgroup; the smallest chain index whose
// auxiliary walk faulted goes to BamState::first_fault (rare: one atomic per such lane).
__global__ __launch_bounds__(256) void bam_keep_filter_kernel(const uint8_t* raw, BamState* bs, const uint32_t* cand, const uint32_t* j0,
                                                               const uint8_t* mark, uint32_t* rec_bytes, uint32_t cap, vgh::BamFilterParams f)
{
    __shared__ uint32_t sh[4];
    const uint32_t n = bs->n_cand;
    if (n > cap) return;
    const BamBytes bytes{raw};
    uint32_t kept = 0, chain = 0;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        uint32_t b = 0;
        if (mark[i]) {
            const uint32_t o = cand[i];
            const uint32_t w12 = bam_ld32(raw, o + 12), w16 = bam_ld32(raw, o + 16), l_seq = bam_ld32(raw, o + 20);
            const int v = vgh::bam_filter_verdict(f, bytes, o, bam_ld32(raw, o), w12 & 0xFFu, (w12 >> 8) & 0xFFu, w16 & 0xFFFFu, w16 >> 16, l_seq,
                                                  (double*)nullptr);
            ++chain;
            if (v == vgh::BAM_FILTER_READ) {
                b = l_seq + 1;
                ++kept;
            } else if (v == vgh::BAM_FILTER_FAULT) {
                atomicMin(&bs->first_fault, i);
            }
            if (j0[i] == n) bs->last = i;
        }
        rec_bytes[i] = b;
    }
    const uint32_t t = block_reduce_add(kept, sh);
    const uint32_t c = block_reduce_add(chain, sh);
    if (threadIdx.x == 0 && t) atomicAdd(&bs->n_kept, t);
    if (threadIdx.x == 0 && c) atomicAdd(&bs->n_chain, c);
}

// B6 with a region list (and whatever filter is set: f holds the defaults where none is): bam_keep_filter_kernel with condition 5 of
// vgmi_bam_filter.h in front of the tag walk.  The interval list is read from device memory, a binary search per lane: a few KB that
// every lane of the chunk walks the same top of, so it stays in the L2.  CIGAR dwords are read only where pos lies in front of an
// interval of its reference, through bam_ld32 like every other field.
__global__ __launch_bounds__(256) void bam_keep_region_kernel(const uint8_t* raw, BamState* bs, const uint32_t* cand, const uint32_t* j0,
                                                               const uint8_t* mark, uint32_t* rec_bytes, uint32_t cap, vgh::BamFilterParams f,
                                                               vgh::BamRegions g)
{
    __shared__ uint32_t sh[4];
    const uint32_t n = bs->n_cand;
    if (n > cap) return;
    const BamBytes bytes{raw};
    uint32_t kept = 0, chain = 0;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        uint32_t b = 0;
        if (mark[i]) {
            const uint32_t o = cand[i];
            const uint32_t w12 = bam_ld32(raw, o + 12), w16 = bam_ld32(raw, o + 16), l_seq = bam_ld32(raw, o + 20);
            const int v = vgh::bam_filter_region_verdict(f, g, bytes, o, bam_ld32(raw, o), w12 & 0xFFu, (w12 >> 8) & 0xFFu, w16 & 0xFFFFu, w16 >> 16,
                                                         l_seq, (int32_t)bam_ld32(raw, o + 4), (int32_t)bam_ld32(raw, o + 8), (double*)nullptr);
            ++chain;
            if (v == vgh::BAM_FILTER_READ) {
                b = l_seq + 1;
                ++kept;
            } else if (v == vgh::BAM_FILTER_FAULT) {
                atomicMin(&bs->first_fault, i);
            }
            if (j0[i] == n) bs->last = i;
        }
        rec_bytes[i] = b;
    }
    const uint32_t t = block_reduce_add(kept, sh);
    const uint32_t c = block_reduce_add(chain, sh);
    if (threadIdx.x == 0 && t) atomicAdd(&bs->n_kept, t);
    if (threadIdx.x == 0 && c) atomicAdd(&bs->n_chain, c);
}

// Behind B6 with a tag bound: the chain is cut at the smallest faulted index.  Chain order is candidate order, so the records at and behind
// it are the marked candidates i >= first_fault: their rec_bytes become 0 and they leave the sums.  `last` becomes the chain
// record in front of the fault -- the marked one whose successor it is -- or none where the fault is the chain's first record.
__global__ __launch_bounds__(256) void bam_cut_kernel(const FqState* st, BamState* bs, const uint32_t* cand, const uint32_t* j0, const uint8_t* mark,
                                                       uint32_t* rec_bytes, uint32_t cap)
{
    __shared__ uint32_t sh[4];
    const uint32_t n = bs->n_cand, ff = bs->first_fault;
    if (n > cap || ff == BAM_NONE) return;   // (uniform)
    uint32_t kept = 0, chain = 0;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        if (!mark[i]) continue;
        if (i < ff) {
            if (j0[i] == ff) bs->last = i;
            continue;
        }
        if (i == ff && cand[i] == st->start) bs->last = BAM_NONE;
        ++chain;
        if (rec_bytes[i]) {
            ++kept;
            rec_bytes[i] = 0;
        }
    }
    const uint32_t t = block_reduce_add(kept, sh);
    const uint32_t c = block_reduce_add(chain, sh);
    if (threadIdx.x == 0 && t) atomicSub(&bs->n_kept, t);
    if (threadIdx.x == 0 && c) atomicSub(&bs->n_chain, c);
}

// B9 with a filter set (SUB: and subsampling): a walk fault stops the device at the faulted record's first byte, which is where the
// cut chain ends -- bam_check would pass that record, its fixed fields are valid.  The stream's totals move on, the per-chunk
// members of the filter are re-armed.
template <bool SUB>
__device__ __forceinline__ void bam_finish_filter(const uint8_t* raw, FqState* st, BamState* bs, const uint32_t* cand, const uint32_t* rec_bytes,
                                                  const uint32_t* out_off, uint32_t n_new, const uint32_t* n_new_dev, uint32_t cap, uint32_t tail_max,
                                                  int32_t n_ref)
{
    if (threadIdx.x || blockIdx.x) return;
    const uint32_t end = bam_end(tail_max, n_new, n_new_dev);
    uint32_t reads = 0, kept = 0, chain = 0, packed = 0, chain_end = st->start, tail = 0;
    if (!st->stopped) {
        const uint32_t n = bs->n_cand;
        if (n > cap) {
            st->stopped = 1;     // more candidates than the arrays hold: nothing of this chunk is taken, the host resumes at its first byte
        } else {
            if (bs->last != BAM_NONE) {
                const uint32_t o = cand[bs->last];
                chain_end = o + 4u + bam_ld32(raw, o);
                reads = bs->n_kept;
                chain = bs->n_chain;
                kept = SUB ? reads - bs->n_dropped : reads;
                packed = out_off[n - 1] + rec_bytes[n - 1];
            }
            if (bs->first_fault != BAM_NONE) {
                st->stopped = 1;     // the record at chain_end has auxiliary fields the walk cannot pass: the host names it
            } else if (chain_end < end) {
                // what follows the chain: the front of a record the next chunk completes, or something the host must judge
                uint32_t block_size = 0;
                const int r = bam_check(raw, chain_end, end, n_ref, &block_size);
                if (r == 1 && (end - chain_end < 4u || block_size <= tail_max - 4u)) tail = end - chain_end;
                else st->stopped = 1;     // not a valid record, or one longer than the carry (whole or not: never a candidate)
            }
        }
    }
    bs->n_dropped = 0;
    bs->n_chain = 0;
    bs->first_fault = BAM_NONE;
    bs->tot_records += chain;
    bs->tot_reads += reads;
    st->n_good = kept;
    st->packed_bytes = packed;
    if (SUB) st->n_seen += reads;
    st->n_records += kept;
    st->n_bases += packed - kept;
    st->consumed += chain_end - st->start;
    st->consumed_end = chain_end;
    st->tail_len = tail;
}

__global__ void bam_finish_filter_kernel(const uint8_t* raw, FqState* st, BamState* bs, const uint32_t* cand, const uint32_t* rec_bytes,
                                         const uint32_t* out_off, uint32_t n_new, const uint32_t* n_new_dev, uint32_t cap, uint32_t tail_max,
                                         int32_t n_ref)
{
    bam_finish_filter<false>(raw, st, bs, cand, rec_bytes, out_off, n_new, n_new_dev, cap, tail_max, n_ref);
}

__global__ void bam_finish_filter_sub_kernel(const uint8_t* raw, FqState* st, BamState* bs, const uint32_t* cand, const uint32_t* rec_bytes,
                                             const uint32_t* out_off, uint32_t n_new, const uint32_t* n_new_dev, uint32_t cap, uint32_t tail_max,
                                             int32_t n_ref)
{
    bam_finish_filter<true>(raw, st, bs, cand, rec_bytes, out_off, n_new, n_new_dev, cap, tail_max, n_ref);
}

// ---- the read filter (vgmi_read_filter.h), off the default path -----------------------------------------------------------------------
__device__ __forceinline__ unsigned long long bam_wave_sum64(unsigned long long v)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// Behind B6 in whichever form, bam_cut_kernel and bam_rank_kernel, in front of B7: one wavefront per candidate with rec_bytes != 0 -- a
// read of the chain in front of any walk fault that subsampling kept, so an accepted one: the class counts go straight to the stream's.
// The length tests first; with a quality test, B8's address arithmetic finds QUAL, a record whose QUAL[0] is 0xff passes (uniform over
// the wavefront), lane i loads QUAL[i], and the sums are those of fq_read_quality_kernel with a table whose clamp is min(byte, 93).
// A failing read's rec_bytes becomes 0, which B7 and B8 pass over; how many, for B9, in FqState::rf_dropped.
__global__ __launch_bounds__(256) void bam_read_filter_kernel(const uint8_t* raw, FqState* st, const BamState* bs, const uint32_t* cand,
                                                              uint32_t* rec_bytes, uint32_t cap, vgh::ReadFilterParams p)
{
    __shared__ uint32_t e_of[256];
    __shared__ uint32_t sh[4];
    const uint32_t n = bs->n_cand;
    if (n > cap) return;   // (uniform)
    e_of[threadIdx.x] = vgh::read_filter_e(vgh::read_filter_q_bam(threadIdx.x));      // (256 threads)
    __syncthreads();
    const bool quality = p.quality();
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = (gridDim.x * blockDim.x) >> 6;
    uint32_t n_short = 0, n_long = 0, n_lf = 0, n_lm = 0;
    for (uint32_t i = wave; i < n; i += n_waves) {
        const uint32_t nb = rec_bytes[i];
        if (!nb) continue;
        const uint32_t l_seq = nb - 1;
        int cls = vgh::read_filter_length_class(p, l_seq);
        if (!cls && quality) {
            const uint32_t o = cand[i];
            const uint32_t s = o + 36u + raw[o + 12] + 4u * (bam_ld32(raw, o + 16) & 0xFFFFu);
            const uint32_t q = s + (l_seq + 1u) / 2u;
            if (raw[q] != 0xFFu) {      // (uniform over the wavefront)
                unsigned long long sum = 0;
                uint32_t low = 0;
                for (uint32_t k = lane; k < l_seq; k += 64) {
                    const uint32_t b = raw[q + k];
                    sum += e_of[b];
                    low += b < p.lowq_below;
                }
                sum = bam_wave_sum64(sum);
                cls = vgh::read_filter_quality_class(p, l_seq, bam_wave_sum64(low), sum);
            }
        }
        if (lane == 0 && cls) {
            rec_bytes[i] = 0;
            n_short += cls == vgh::READ_SHORT;
            n_long += cls == vgh::READ_LONG;
            n_lf += cls == vgh::READ_LOW_FRACTION;
            n_lm += cls == vgh::READ_LOW_MEAN;
        }
    }
    const uint32_t ts = block_reduce_add(n_short, sh), tl = block_reduce_add(n_long, sh);
    const uint32_t tf = block_reduce_add(n_lf, sh), tm = block_reduce_add(n_lm, sh);
    if (threadIdx.x) return;
    if (ts) atomicAdd(&st->n_short, (unsigned long long)ts);
    if (tl) atomicAdd(&st->n_long, (unsigned long long)tl);
    if (tf) atomicAdd(&st->n_low_fraction, (unsigned long long)tf);
    if (tm) atomicAdd(&st->n_low_mean, (unsigned long long)tm);
    if (ts + tl + tf + tm) atomicAdd(&st->rf_dropped, ts + tl + tf + tm);
}

// B9 with a read filter, whatever else is set: bam_finish_filter's bookkeeping (without a record filter its sums stay 0 and nothing
// faults), n_seen moves on by the chain's reads, and the reads the rule dropped leave n_records while n_seen and tot_reads stay the
// passing records'
__global__ void bam_finish_rf_kernel(const uint8_t* raw, FqState* st, BamState* bs, const uint32_t* cand, const uint32_t* rec_bytes,
                                     const uint32_t* out_off, uint32_t n_new, const uint32_t* n_new_dev, uint32_t cap, uint32_t tail_max, int32_t n_ref)
{
    if (threadIdx.x || blockIdx.x) return;
    const uint32_t end = bam_end(tail_max, n_new, n_new_dev);
    uint32_t reads = 0, kept = 0, chain = 0, packed = 0, chain_end = st->start, tail = 0;
    if (!st->stopped) {
        const uint32_t n = bs->n_cand;
        if (n > cap) {
            st->stopped = 1;     // more candidates than the arrays hold: nothing of this chunk is taken, the host resumes at its first byte
        } else {
            if (bs->last != BAM_NONE) {
                const uint32_t o = cand[bs->last];
                chain_end = o + 4u + bam_ld32(raw, o);
                reads = bs->n_kept;
                chain = bs->n_chain;
                kept = reads - bs->n_dropped - st->rf_dropped;
                packed = out_off[n - 1] + rec_bytes[n - 1];
            }
            if (bs->first_fault != BAM_NONE) {
                st->stopped = 1;     // the record at chain_end has auxiliary fields the walk cannot pass: the host names it
            } else if (chain_end < end) {
                // what follows the chain: the front of a record the next chunk completes, or something the host must judge
                uint32_t block_size = 0;
                const int r = bam_check(raw, chain_end, end, n_ref, &block_size);
                if (r == 1 && (end - chain_end < 4u || block_size <= tail_max - 4u)) tail = end - chain_end;
                else st->stopped = 1;     // not a valid record, or one longer than the carry (whole or not: never a candidate)
            }
        }
    }
    bs->n_dropped = 0;
    bs->n_chain = 0;
    bs->first_fault = BAM_NONE;
    bs->tot_records += chain;
    bs->tot_reads += reads;
    st->rf_dropped = 0;
    st->n_good = kept;
    st->packed_bytes = packed;
    st->n_seen += reads;
    st->n_records += kept;
    st->n_bases += packed - kept;
    st->consumed += chain_end - st->start;
    st->consumed_end = chain_end;
    st->tail_len = tail;
}

// B10: the unconsumed tail goes in front of the next chunk's landing area, and the per-chunk state is re-armed
__global__ __launch_bounds__(256) void bam_carry_kernel(const uint8_t* raw, uint8_t* raw_next, FqState* st, BamState* bs, uint32_t tail_max)
{
    const uint32_t tail = st->tail_len, from = st->consumed_end;
    for (uint32_t i = threadIdx.x; i < tail; i += blockDim.x) raw_next[tail_max - tail + i] = raw[from + i];
    __syncthreads();
    if (threadIdx.x == 0) {
        st->start = tail_max - tail;
        bs->n_cand = 0;
        bs->last = BAM_NONE;
        bs->n_kept = 0;
    }
}

__global__ void bam_init_kernel(BamState* bs, unsigned long long header_bytes)
{
    if (threadIdx.x || blockIdx.x) return;
    *bs = BamState{};
    bs->hdr_left = header_bytes;
    bs->last = BAM_NONE;
    bs->first_fault = BAM_NONE;
}

// ---- launchers ------------------------------------------------------------------------------------------------------------------
hipError_t launch_bam_init(BamState* bs, unsigned long long header_bytes, hipStream_t s)
{
    hipLaunchKernelGGL(bam_init_kernel, dim3(1), dim3(1), 0, s, bs, header_bytes);
    return hipGetLastError();
}

hipError_t launch_bam_chunk(const BamBuffers& b, uint32_t n_new, hipStream_t s, const uint32_t* n_new_dev)
{
    const uint32_t end = b.tail_max + n_new;
    const uint32_t n_tiles = (end + BAM_TILE - 1) / BAM_TILE;
    const uint32_t n_rblk = b.cap_cand / 1024u + 1;
    const uint32_t grid = (b.cap_cand + 256u) / 256u < BAM_GRID ? (b.cap_cand + 256u) / 256u : BAM_GRID;
    hipLaunchKernelGGL(bam_begin_kernel, dim3(1), dim3(1), 0, s, b.state, b.bam, b.tail_max, n_new, n_new_dev);
    hipLaunchKernelGGL(bam_count_kernel, dim3(n_tiles), dim3(256), 0, s, b.raw, b.state, b.tail_max, n_new, n_new_dev, b.n_ref, b.tile);
    hipError_t e = launch_scan_small(b.tile, n_tiles, &b.bam->n_cand, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(bam_cand_kernel, dim3(n_tiles), dim3(256), 0, s, b.raw, b.state, b.bam, b.tail_max, n_new, n_new_dev, b.n_ref, b.tile, b.cand,
                       b.cap_cand);
    hipLaunchKernelGGL(bam_link_kernel, dim3(grid), dim3(256), 0, s, b.raw, b.state, b.bam, b.cand, b.j0, b.mark, b.cap_cand);
    // rounds while 2^r < n: ceil(log2(cap + 1)) launched, those beyond the chunk's candidates return at once
    const uint32_t* src = b.j0;
    for (uint32_t r = 0; (1ull << r) <= b.cap_cand; ++r) {
        uint32_t* dst = src == b.ja ? b.jb : b.ja;
        hipLaunchKernelGGL(bam_jump_kernel, dim3(grid), dim3(256), 0, s, b.bam, src, dst, b.mark, r, b.cap_cand);
        src = dst;
    }
    const bool filtered = b.filt.on || b.n_regions;      // B9's filter forms keep the sums either rule needs
    const vgh::BamFilterParams filt = b.filt.on ? b.filt : vgh::bam_filter_params();
    if (b.n_regions) {
        hipLaunchKernelGGL(bam_keep_region_kernel, dim3(grid), dim3(256), 0, s, b.raw, b.bam, b.cand, b.j0, b.mark, b.rec_bytes, b.cap_cand, filt,
                           vgh::BamRegions{b.regions, b.n_regions, b.regions_unplaced});
        if (filt.tag)
            hipLaunchKernelGGL(bam_cut_kernel, dim3(grid), dim3(256), 0, s, b.state, b.bam, b.cand, b.j0, b.mark, b.rec_bytes, b.cap_cand);
    } else if (b.filt.on) {
        hipLaunchKernelGGL(bam_keep_filter_kernel, dim3(grid), dim3(256), 0, s, b.raw, b.bam, b.cand, b.j0, b.mark, b.rec_bytes, b.cap_cand, b.filt);
        if (b.filt.tag)      // (without a tag bound no auxiliary byte is read: nothing can fault)
            hipLaunchKernelGGL(bam_cut_kernel, dim3(grid), dim3(256), 0, s, b.state, b.bam, b.cand, b.j0, b.mark, b.rec_bytes, b.cap_cand);
    } else {
        hipLaunchKernelGGL(bam_keep_kernel, dim3(grid), dim3(256), 0, s, b.raw, b.bam, b.cand, b.j0, b.mark, b.rec_bytes, b.cap_cand);
    }
    if (b.sub.on) {
        hipLaunchKernelGGL(bam_rank_kernel, dim3(n_rblk), dim3(1024), 0, s, b.rec_bytes, b.state, b.bam, b.block_sum, 0, b.cap_cand, b.sub.seed,
                           b.sub.threshold);
        e = launch_scan_small(b.block_sum, n_rblk, nullptr, s);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(bam_rank_kernel, dim3(n_rblk), dim3(1024), 0, s, b.rec_bytes, b.state, b.bam, b.block_sum, 1, b.cap_cand, b.sub.seed,
                           b.sub.threshold);
    }
    if (b.rf.on)
        hipLaunchKernelGGL(bam_read_filter_kernel, dim3(BAM_GRID), dim3(256), 0, s, b.raw, b.state, b.bam, b.cand, b.rec_bytes, b.cap_cand, b.rf);
    hipLaunchKernelGGL(bam_scan_blocks_kernel, dim3(n_rblk), dim3(1024), 0, s, b.rec_bytes, b.bam, b.block_sum, b.out_off, 0, b.cap_cand);
    e = launch_scan_small(b.block_sum, n_rblk, nullptr, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(bam_scan_blocks_kernel, dim3(n_rblk), dim3(1024), 0, s, b.rec_bytes, b.bam, b.block_sum, b.out_off, 1, b.cap_cand);
    if (b.min_qual)
        hipLaunchKernelGGL(bam_decode_mask_kernel, dim3(BAM_GRID), dim3(256), 0, s, b.raw, b.state, b.bam, b.cand, b.rec_bytes, b.out_off, b.packed,
                           b.cap_cand, b.min_qual);
    else hipLaunchKernelGGL(bam_decode_kernel, dim3(BAM_GRID), dim3(256), 0, s, b.raw, b.bam, b.cand, b.rec_bytes, b.out_off, b.packed, b.cap_cand);
    if (b.rf.on)
        hipLaunchKernelGGL(bam_finish_rf_kernel, dim3(1), dim3(1), 0, s, b.raw, b.state, b.bam, b.cand, b.rec_bytes, b.out_off, n_new, n_new_dev, b.cap_cand,
                           b.tail_max, b.n_ref);
    else if (filtered && b.sub.on)
        hipLaunchKernelGGL(bam_finish_filter_sub_kernel, dim3(1), dim3(1), 0, s, b.raw, b.state, b.bam, b.cand, b.rec_bytes, b.out_off, n_new, n_new_dev,
                           b.cap_cand, b.tail_max, b.n_ref);
    else if (filtered)
        hipLaunchKernelGGL(bam_finish_filter_kernel, dim3(1), dim3(1), 0, s, b.raw, b.state, b.bam, b.cand, b.rec_bytes, b.out_off, n_new, n_new_dev,
                           b.cap_cand, b.tail_max, b.n_ref);
    else if (b.sub.on)
        hipLaunchKernelGGL(bam_finish_sub_kernel, dim3(1), dim3(1), 0, s, b.raw, b.state, b.bam, b.cand, b.rec_bytes, b.out_off, n_new, n_new_dev,
                           b.cap_cand, b.tail_max, b.n_ref);
    else
        hipLaunchKernelGGL(bam_finish_kernel, dim3(1), dim3(1), 0, s, b.raw, b.state, b.bam, b.cand, b.rec_bytes, b.out_off, n_new, n_new_dev, b.cap_cand,
                           b.tail_max, b.n_ref);
    hipLaunchKernelGGL(bam_carry_kernel, dim3(1), dim3(256), 0, s, b.raw, b.raw_next, b.state, b.bam, b.tail_max);
    return hipGetLastError();
}

}  // namespace vgk
