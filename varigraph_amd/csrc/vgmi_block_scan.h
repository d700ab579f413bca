// vgmi_block_scan.h -- workgroup-wide sum and exclusive scan (wave64 shuffles + one LDS slot per wave), shared by the record
// parsers (vgmi_fastq.hip, vgmi_bam.hip)
#ifndef VGMI_BLOCK_SCAN_H
#define VGMI_BLOCK_SCAN_H
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace vgk {

__device__ __forceinline__ uint32_t block_reduce_add(uint32_t v, uint32_t* sh)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    if ((threadIdx.x & 63u) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    uint32_t t = 0;
    for (uint32_t i = 0; i < (blockDim.x >> 6); ++i) t += sh[i];
    __syncthreads();
    return t;
}

// exclusive prefix of v over the block's threads (blockDim.x <= 1024); *total = block sum
__device__ __forceinline__ uint32_t block_scan_excl(uint32_t v, uint32_t* sh, uint32_t* total)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t inc = v;
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t n = __shfl_up(inc, o);
        if (lane >= (uint32_t)o) inc += n;
    }
    if (lane == 63) sh[wave] = inc;
    __syncthreads();
    uint32_t base = 0, tot = 0;
    for (uint32_t i = 0; i < (blockDim.x >> 6); ++i) {
        if (i < wave) base += sh[i];
        tot += sh[i];
    }
    __syncthreads();
    if (total) *total = tot;
    return base + inc - v;
}

}  // namespace vgk

#endif
