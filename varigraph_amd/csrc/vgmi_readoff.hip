// vgmi_readoff.hip -- where the reads of a '\n'-joined read block start, found on the device (gfx950).
//
// Even k counts read by read (seq_kernel, even_debit_kernel: vgmi_kernels.hip), so behind the device-side readers -- whose read block
// and its length never leave the device -- the reads' offsets and their number must be there too.  Every reader (vgmi_fastq.hip,
// vgmi_fasta.hip, vgmi_bam.hip) ends a read with '\n' and writes no other '\n' into the block (a base is never one; the BAM decoder's
// sixteen letters hold none), so the offsets are the positions behind the block's newlines, whatever the container was:
//   R1 newlines per 16 KiB tile -> R2 scan of the tiles (fq_scan_small_kernel; its total is the number of reads) -> R3 the offsets in order.
// Launched for even k only: a stream over an odd-k table launches none of this, and the readers themselves are untouched.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vgmi_block_scan.h"
#include "vgmi_kernels.h"

namespace vgk {

#define RO_PIECES 4u                       // 16-byte pieces per thread, 4 KiB apart
#define RO_TILE (4096u * RO_PIECES)        // bytes per workgroup

// bit j of the result = byte j of the 16 is a '\n' and lies in front of `n`
__device__ __forceinline__ uint32_t ro_nl_mask(const uint4 v, uint64_t off, uint64_t n)
{
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    uint32_t m = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const uint32_t x = w[i] ^ 0x0A0A0A0Au;
        const uint32_t z = ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu);      // bit 7 of a byte set iff the byte is zero (exact)
        m |= (((z >> 7) & 1u) | ((z >> 14) & 2u) | ((z >> 21) & 4u) | ((z >> 28) & 8u)) << (4 * i);
    }
    return off + 16 <= n ? m : m & ((1u << (uint32_t)(n - off)) - 1u);
}

// (the block's allocation has 256 bytes of slack behind the largest block: a 16-byte load that starts in front of n stays inside)
__device__ __forceinline__ uint4 ro_load(const uint8_t* packed, uint64_t off, uint64_t n)
{
    return off < n ? *reinterpret_cast<const uint4*>(packed + off) : make_uint4(0x41414141u, 0x41414141u, 0x41414141u, 0x41414141u);
}

// R1: the launch covers the host's bound on the block's length; a workgroup past the real end writes its zero and returns
__global__ __launch_bounds__(256) void ro_count_kernel(const uint8_t* __restrict__ packed, const unsigned long long* __restrict__ n_bytes_dev,
                                                       uint32_t* __restrict__ tile_nl)
{
    __shared__ uint32_t sh[4];
    const uint64_t n = *n_bytes_dev, t0 = (uint64_t)blockIdx.x * RO_TILE;
    if (t0 >= n) {      // (uniform)
        if (threadIdx.x == 0) tile_nl[blockIdx.x] = 0;
        return;
    }
    uint4 v[RO_PIECES];
#pragma unroll
    for (uint32_t j = 0; j < RO_PIECES; ++j) v[j] = ro_load(packed, t0 + j * 4096u + threadIdx.x * 16u, n);
    uint32_t cnt = 0;
#pragma unroll
    for (uint32_t j = 0; j < RO_PIECES; ++j) {
        const uint64_t off = t0 + j * 4096u + threadIdx.x * 16u;
        if (off < n) cnt += __popc(ro_nl_mask(v[j], off, n));
    }
    const uint32_t t = block_reduce_add(cnt, sh);
    if (threadIdx.x == 0) tile_nl[blockIdx.x] = t;
}

// R3: read r + 1 starts behind the r-th newline; read_off[n_reads] is the block's length
__global__ __launch_bounds__(256) void ro_offsets_kernel(const uint8_t* __restrict__ packed, const unsigned long long* __restrict__ n_bytes_dev,
                                                         const uint32_t* __restrict__ tile_base, uint64_t* __restrict__ read_off, uint64_t cap_reads)
{
    __shared__ uint32_t sh[4];
    const uint64_t n = *n_bytes_dev, t0 = (uint64_t)blockIdx.x * RO_TILE;
    if (blockIdx.x == 0 && threadIdx.x == 0) read_off[0] = 0;
    if (t0 >= n) return;      // (uniform)
    uint32_t m[RO_PIECES];
#pragma unroll
    for (uint32_t j = 0; j < RO_PIECES; ++j) {
        const uint64_t off = t0 + j * 4096u + threadIdx.x * 16u;
        m[j] = off < n ? ro_nl_mask(ro_load(packed, off, n), off, n) : 0u;
    }
    uint64_t base = tile_base[blockIdx.x];
#pragma unroll
    for (uint32_t j = 0; j < RO_PIECES; ++j) {      // piece by piece: the newlines of a tile in order
        uint32_t tot, mm = m[j];
        uint64_t pos = base + block_scan_excl(__popc(mm), sh, &tot);
        base += tot;
        const uint64_t off = t0 + j * 4096u + threadIdx.x * 16u;
        while (mm) {
            const uint32_t q = __builtin_ctz(mm);
            mm &= mm - 1;
            ++pos;
            if (pos <= cap_reads) read_off[pos] = off + q + 1;
        }
    }
}

size_t read_offsets_tiles(uint64_t n_bytes_bound) { return (size_t)((n_bytes_bound + RO_TILE - 1) / RO_TILE); }

hipError_t launch_read_offsets(const uint8_t* packed, uint64_t n_bytes_bound, const unsigned long long* n_bytes_dev, uint32_t* tile, uint64_t* read_off,
                               uint64_t cap_reads, unsigned long long* n_reads_dev, hipStream_t st)
{
    const uint32_t n_tiles = (uint32_t)read_offsets_tiles(n_bytes_bound);
    if (n_tiles == 0) return hipSuccess;
    hipLaunchKernelGGL(ro_count_kernel, dim3(n_tiles), dim3(256), 0, st, packed, n_bytes_dev, tile);
    // (the total is 32 bits wide and goes to the low word of *n_reads_dev, whose high word the owner zeroed once)
    hipError_t e = launch_scan_small(tile, n_tiles, reinterpret_cast<uint32_t*>(n_reads_dev), st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(ro_offsets_kernel, dim3(n_tiles), dim3(256), 0, st, packed, n_bytes_dev, tile, read_off, cap_reads);
    return hipGetLastError();
}

}  // namespace vgk
