// vgmi_inflate.hip -- block-gzip (BGZF) members inflated on the device (gfx950), one wavefront per member.
//
// What it replaces: zlib's inflate behind gzread (include/kseq.h:59-72 over gzFile, src/fastq_kmer.cpp:74-78) for files
// written by bgzip / htslib: a BGZF file is a series of complete gzip members of at most 64 KiB (the 'BC' extra field
// carries each member's size), so the members are independent DEFLATE streams (RFC 1951) -- the host only walks the
// headers and ships compressed bytes; every member becomes text in its place of the chunk the FASTQ kernels
// (vgmi_fastq.hip) parse.  A member the kernel cannot vouch for -- bad Huffman code, output that does not match ISIZE
// or CRC-32 (RFC 1952) -- is reported, the chunk is cut in front of it and the host decoder (csrc/host/fast_inflate.cpp,
// pinned against zlib) takes the stream over there; nothing the device emits is unchecked.
//
// The DEFLATE decoder itself -- block headers, code tables, the two batch forms, the one-symbol path -- is inf_block of
// vgmi_inflate_dev.h, shared with vgmi_gunzip.hip.  This file holds what is the member's own: BgzfSink (input of any alignment,
// bytes out, the member's two lengths as the limits) and the kernel around it -- a loop over the member's blocks, then ISIZE and
// CRC-32.
//
// Shape of the decoder (round 4).  DEFLATE decoding is serial inside a member: where a symbol starts is known only once the
// symbol before it is decoded.  Rounds 2-3 ran that chain one look-up at a time in scalar registers (one LDS round trip and
// ~14 scalar instructions per one to three output bytes: latency-bound at 58 cycles per byte and SIMD).  Now a BATCH of 64 bit
// positions is decoded at once: lane i decodes the symbol that would start at bit (position + i) -- one gather from the
// literal/length table (entries hold up to three literals), one from the distance table -- and only then a short scalar walk
// hops from symbol start to symbol start over the lanes' results (one v_readlane per symbol), handing every real symbol its
// output offset.  Literals of the whole batch are written in one step; matches are copied one after the other, each copy
// 64 bytes wide (a match of length n from distance d is the periodic extension of the d bytes before it).  Output goes to a
// 2 KiB LDS ring (the LZ77 window for near matches) and leaves for global memory in aligned 256-byte blocks.  Codes longer
// than the tables' index, stored blocks and block headers take a scalar path, one symbol at a time.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "vgmi_kernels.h"

#include "vgmi_inflate_dev.h"

namespace vgk {

// ---- CRC-32 (gzip polynomial, reflected) ---------------------------------------------------------------------------
#define INF_POLY 0xEDB88320u
// a(x) * b(x) mod p(x); bit 31 = x^0 (the arithmetic of zlib's crc32_combine)
__device__ __forceinline__ uint32_t gf2_mul(uint32_t a, uint32_t b)
{
    uint32_t p = 0;
    for (uint32_t m = 1u << 31; m; m >>= 1) {
        if (a & m) p ^= b;
        b = (b & 1u) ? (b >> 1) ^ INF_POLY : b >> 1;
    }
    return p;
}
// x^(8 n) mod p(x)
__device__ __forceinline__ uint32_t gf2_x8n(uint32_t n)
{
    uint32_t p = 1u << 31, sq = 0x00800000u;   // x^8
    for (; n; n >>= 1) {
        if (n & 1u) p = gf2_mul(sq, p);
        sq = gf2_mul(sq, sq);
    }
    return p;
}

// What a block-gzip member gives the block decoder (vgmi_inflate_dev.h: inf_block).  The member's deflate bytes start at any
// address; its text goes to its place in the chunk as bytes, no farther than ISIZE.
template <bool WIDE>
struct BgzfSink {
    typedef InfWideT<uint8_t, 4096> WideTables;
    typedef typename std::conditional<WIDE, WideTables, InfTables>::type Tables;
    typedef uint8_t Ring;
    static constexpr uint32_t kRing = WIDE ? WideTables::kRing : INF_RING, kNear = WIDE ? WideTables::kNear : INF_NEAR;
    static constexpr uint32_t kStored = 256u;
    static constexpr uint32_t back_ok = 0u;        // a member's matches reach no farther than its own first byte
    Tables& t;
    const uint32_t lane;
    const uint8_t* const in;
    const uint32_t in_len;                         // deflate bytes (header and trailer stripped by the host walk)
    // the batches read the input as aligned 32-bit words: in4 + lead_bits is the member's first bit
    const uint32_t* const in4;
    const uint32_t lead_bits;
    // the wide batches read the input through a descriptor: words behind the member's last read as zero
    const __amdgpu_buffer_rsrc_t irsrc;
    uint8_t* const out;
    const uint32_t cap;                            // ISIZE
    const __amdgpu_buffer_rsrc_t orsrc;            // stores at offsets >= ISIZE are dropped by the hardware
    uint32_t* const ring32;
    const uint32_t head;                           // bytes in front of the first aligned word of the output
    uint32_t flushed = 0;                          // output bytes that are in global memory

    __device__ __forceinline__ BgzfSink(Tables& t_, uint32_t lane_, const uint8_t* in_, uint32_t in_len_, uint8_t* out_, uint32_t out_len)
        : t(t_), lane(lane_), in(in_), in_len(in_len_), in4(reinterpret_cast<const uint32_t*>((uintptr_t)in_ & ~(uintptr_t)3)),
          lead_bits(8u * (uint32_t)((uintptr_t)in_ & 3u)),
          irsrc(__builtin_amdgcn_make_buffer_rsrc(const_cast<uint32_t*>(in4), 0, (int)((lead_bits / 8u + in_len_ + 3u) & ~3u), 0x00020000)), out(out_), cap(out_len),
          orsrc(__builtin_amdgcn_make_buffer_rsrc(out_, 0, (int)out_len, 0x00020000)), ring32(reinterpret_cast<uint32_t*>(t_.ring)),
          head((4u - (uint32_t)((uintptr_t)out_ & 3u)) & 3u)
    {
    }

    __device__ __forceinline__ uint32_t stored_overrun(uint32_t src, uint32_t len, uint32_t op) const { return src + len > in_len || op + len > cap ? 3u : 0u; }
    // full: more text than ISIZE says; or a damaged stream running away over the input
    __device__ __forceinline__ uint32_t overrun(bool full, uint32_t bp, uint32_t) const { return full || (bp >> 3) > in_len + 8u ? 3u : 0u; }
    __device__ __forceinline__ uint32_t slow_overrun(uint32_t) const { return 0u; }
    __device__ __forceinline__ void block_end(uint32_t bp, uint32_t& err) const
    {
        if ((bp + 7u) / 8u > in_len) err = 3;      // the block ran past the member's deflate bytes
    }
    // ring -> global memory: whole 256-byte blocks of aligned words (all of it at the end)
    __device__ __forceinline__ void flush(uint32_t op, bool all)
    {
        if (flushed < head && (op >= head || all)) {
            const uint32_t n = op < head ? op : head;
            if (lane < n) __builtin_amdgcn_raw_buffer_store_b8(t.ring[lane], orsrc, lane, 0, 0);
            flushed = n;
        }
        while (flushed >= head && op - flushed >= 256u) {
            const uint32_t r = (flushed + 4u * lane) & (kRing - 1u);
            const uint32_t w0 = ring32[r >> 2], w1 = ring32[((r >> 2) + 1u) & (kRing / 4u - 1u)];
            const uint32_t v = __builtin_amdgcn_alignbyte(w1, w0, r & 3u);
            __builtin_amdgcn_raw_buffer_store_b32(v, orsrc, flushed + 4u * lane, 0, 0);
            flushed += 256u;
        }
        if (all)
            while (flushed < op) {
                const uint32_t p = flushed + lane;
                if (p < op) __builtin_amdgcn_raw_buffer_store_b8(t.ring[p & (kRing - 1u)], orsrc, p, 0, 0);
                flushed = flushed + 64u < op ? flushed + 64u : op;
            }
    }
    // one LZ77 match at output position P (every earlier byte is in the ring, or in global memory when far): 64 bytes per step
    __device__ __forceinline__ void copy_match(uint32_t P, uint32_t len, uint32_t dist)
    {
        if (dist <= kNear) {
            for (uint32_t i = lane; i < len; i += 64) {
                const uint8_t b = t.ring[(P - dist + (dist >= len ? i : i % dist)) & (kRing - 1u)];
                t.ring[(P + i) & (kRing - 1u)] = b;
            }
        } else {
            // far: the source is in front of everything still unflushed (kNear > the ring's unflushed part + a batch); read it
            // back once the wavefront's stores have landed (its own stores and loads go through the same vector cache; an
            // agent-scope fence here writes the whole L2 back and made the kernel 15 x slower -- whatever this read could get
            // wrong, the CRC of the kernel's epilogue catches and the host decoder redoes)
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            const uint8_t* const src = out + P - dist;
            for (uint32_t i = lane; i < len; i += 64) t.ring[(P + i) & (kRing - 1u)] = src[dist >= len ? i : i % dist];
        }
        inf_sync();
    }
    __device__ __forceinline__ bool matches(uint32_t n_match, uint32_t op) { return infw_matches<Tables, uint8_t, false>(t, n_match, op, out, 0u, lane); }
};

// One member per wavefront.  status[m]: 0 = good, else the reason (1 code lengths, 2 bad symbol / distance, 3 output or
// input overrun, 4 length != ISIZE, 5 CRC-32, 6 stored-block header, 7 reserved block type).
template <bool WIDE>
__global__ __launch_bounds__(64 * INF_WAVES, WIDE ? 3 : 4) void bgzf_inflate_kernel(const uint8_t* __restrict__ comp, const BgzfMember* __restrict__ members,
                                                                                uint32_t n_members, uint8_t* __restrict__ out_base, uint32_t* __restrict__ status,
                                                                                const uint32_t* __restrict__ crc_table)
{
    typedef typename BgzfSink<WIDE>::Tables Tables;
    __shared__ Tables tabs[INF_WAVES];
    __shared__ uint32_t s_crc[256];
    for (uint32_t i = threadIdx.x; i < 256; i += blockDim.x) s_crc[i] = crc_table[i];
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave_in_block = uni(threadIdx.x >> 6);
    const uint32_t m = blockIdx.x * INF_WAVES + wave_in_block;
    if (m >= n_members) return;
    Tables& t = tabs[wave_in_block];
    uint8_t* const out = out_base + uni(members[m].u_off);
    const uint32_t out_len = uni(members[m].u_len);      // ISIZE
    const uint32_t want_crc = uni(members[m].crc);
    BgzfSink<WIDE> sink(t, lane, comp + uni(members[m].c_off), uni(members[m].c_len), out, out_len);

    // ---- wave-uniform decoder state ----
    uint32_t bp = 0;            // bits of the member's deflate data consumed
    uint32_t op = 0;            // output bytes produced (in the ring, or flushed)
    uint32_t err = 0;
    bool last = false;
    while (!last && !err) inf_block<WIDE>(sink, bp, op, err, last);
    if (!err && op != out_len) err = 4;
    sink.flush(op, true);
    if (!err && out_len) {
        // CRC-32 of the output: one slice per lane, then crc(A || B) = crc(A) * x^(8 |B|) + crc(B) in GF(2)[x] / p(x).  The
        // bytes are read back from global memory once the wavefront's stores have landed.
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        const uint32_t slice = (out_len + 63u) / 64u;
        const uint32_t b = lane * slice < out_len ? lane * slice : out_len;
        const uint32_t e = b + slice < out_len ? b + slice : out_len;
        uint32_t c = 0xFFFFFFFFu;
        {
            // sixteen bytes a step, as four aligned words fetched together (one byte load a step, each waited for, was 0.4 of a
            // member's 3 ms)
            uint32_t i = b;
            for (; i < e && ((uintptr_t)(out + i) & 3u); ++i) c = s_crc[(c ^ out[i]) & 0xFFu] ^ (c >> 8);
            for (; i + 16u <= e; i += 16u) {
                const uint32_t* const w = reinterpret_cast<const uint32_t*>(out + i);
                const uint32_t w0 = w[0], w1 = w[1], w2 = w[2], w3 = w[3];
#pragma unroll
                for (uint32_t k = 0; k < 16u; ++k) {
                    const uint32_t word = k < 4 ? w0 : k < 8 ? w1 : k < 12 ? w2 : w3;
                    c = s_crc[(c ^ (word >> (8u * (k & 3u)))) & 0xFFu] ^ (c >> 8);
                }
            }
            for (; i < e; ++i) c = s_crc[(c ^ out[i]) & 0xFFu] ^ (c >> 8);
        }
        t.lit[lane] = ~c;      // (the decode tables are no longer needed)
        inf_sync();
        if (lane == 0) {
            const uint32_t x_full = gf2_x8n(slice);
            uint32_t crc = t.lit[0];
            for (uint32_t i = 1; i < 64; ++i) {
                const uint32_t bi = i * slice;
                if (bi >= out_len) break;
                const uint32_t li = bi + slice <= out_len ? slice : out_len - bi;
                crc = gf2_mul(li == slice ? x_full : gf2_x8n(li), crc) ^ t.lit[i];
            }
            if (crc != want_crc) err = 5;
        }
        err = uni(err);
    }
    if (lane == 0) status[m] = err;
}

// first bad member of the batch (n_members if all are good), and the chunk length the FASTQ kernels may parse
__global__ void bgzf_verdict_kernel(const BgzfMember* members, const uint32_t* status, uint32_t n_members, BgzfVerdict* v)
{
    __shared__ uint32_t first;
    if (threadIdx.x == 0) first = n_members;
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < n_members; i += blockDim.x)
        if (status[i]) atomicMin(&first, i);
    __syncthreads();
    if (threadIdx.x == 0) {
        if (v->first_bad_batch == 0xFFFFFFFFu && first < n_members) {   // sticky: only the first failure of the stream counts
            v->first_bad_batch = v->batches;
            v->first_bad_member = first;
            v->reason = status[first];
        }
        // text that may be parsed: everything in front of the first bad member (nothing once an earlier batch failed)
        uint32_t good_bytes = 0;
        if (v->first_bad_batch == 0xFFFFFFFFu) good_bytes = n_members ? members[n_members - 1].u_off + members[n_members - 1].u_len : 0;
        else if (v->first_bad_batch == v->batches) good_bytes = members[first].u_off;
        v->good_bytes = good_bytes;
        v->batches++;
    }
}

// wavefronts of the inflate kernel the device holds at once (a member each): a commit of a whole multiple leaves no round of
// wavefronts half empty
uint32_t bgzf_wave_slots(int n_cu)
{
    const bool wide = inf_wide_form();
    int nb = 0;
    const hipError_t e = wide ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, bgzf_inflate_kernel<true>, 64 * INF_WAVES, 0)
                              : hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, bgzf_inflate_kernel<false>, 64 * INF_WAVES, 0);
    if (e != hipSuccess || nb <= 0) {
        (void)hipGetLastError();
        return 0;
    }
    return (uint32_t)nb * INF_WAVES * (uint32_t)n_cu;
}

hipError_t launch_bgzf_inflate(const uint8_t* comp, const BgzfMember* members, uint32_t n_members, uint8_t* out_base, uint32_t* status,
                               const uint32_t* crc_table, BgzfVerdict* verdict, hipStream_t s)
{
    const bool wide = inf_wide_form();
    if (n_members) {
        if (wide)
            hipLaunchKernelGGL(bgzf_inflate_kernel<true>, dim3((n_members + INF_WAVES - 1) / INF_WAVES), dim3(64 * INF_WAVES), 0, s, comp, members, n_members, out_base,
                               status, crc_table);
        else
            hipLaunchKernelGGL(bgzf_inflate_kernel<false>, dim3((n_members + INF_WAVES - 1) / INF_WAVES), dim3(64 * INF_WAVES), 0, s, comp, members, n_members, out_base,
                               status, crc_table);
    }
    hipLaunchKernelGGL(bgzf_verdict_kernel, dim3(1), dim3(256), 0, s, members, status, n_members, verdict);
    return hipGetLastError();
}

}  // namespace vgk
