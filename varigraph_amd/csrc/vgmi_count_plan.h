// vgmi_count_plan.h -- how a read block is split between a fast count kernel and the exact tail, and which launches count it.
//
// Pure: no HIP calls, no context, no environment.  The host (launch_count in vgmi_api.cpp) and the kernels that find their share of a
// block whose length lives in device memory (rows_kernel, the DEV forms of seq_kernel and of the debit kernels) read the split from
// here, so the debit pass and the tail cannot disagree about a row boundary.  The fast kernels count their complete rows themselves
// (n / 768; n / 1536 and n / 2048 pairs: one line each, kept as they are for their instruction streams); the CPU suite's check
// (tests/native/count_plan_check.cpp) holds vg_row_split against those formulas and against the rows' coverage lane by lane.
#ifndef VGMI_COUNT_PLAN_H
#define VGMI_COUNT_PLAN_H

#include <stdint.h>

#include "vgmi_device.h"

// the fast kernel in front of the exact tail: the values of RowParams::tail27
enum vg_fast : uint32_t {
    VG_FAST_NONE = 0,
    VG_FAST_ROWS27 = 1,    // count27_kernel: pairs of 768-byte rows, lane L of a row covers the ends 12 L - 1 .. 12 L + 10
    VG_FAST_TABLE = 2,     // context table / grid-16-mer table (count27c_kernel, count27x_kernel): single 768-byte rows, the same ends
    VG_FAST_SMALL27 = 3,   // count27s_kernel, k = 27: pairs of 1 024-byte rows, lane L covers the ends 16 L - 1 .. 16 L + 14
    VG_FAST_SMALLK = 4,    // count27s_kernel<true, K < 27>: the same rows, lane L covers 16 L .. 16 L + 15 -- every end inside its rows
};

// row_end: the complete rows the fast kernel walks (even where it walks pairs).  emit_from: the first stream position whose k-mer END
// the fast kernel does not cover -- the exact tail counts the ends at or behind it, the debit pass of even k the positions in front.
struct vg_split {
    uint64_t row_end, emit_from;
};

VG_HD vg_split vg_row_split(uint32_t fast, uint64_t n_bytes)
{
    if (fast == VG_FAST_NONE) return {0, 0};
    const uint64_t row_bytes = fast >= VG_FAST_SMALL27 ? 1024u : 768u;      // (every division by a constant: the kernels call this)
    const uint64_t row_end = fast == VG_FAST_TABLE ? n_bytes / 768 : fast >= VG_FAST_SMALL27 ? (n_bytes / 2048) * 2 : (n_bytes / 1536) * 2;
    return {row_end, row_end ? row_end * row_bytes - (fast == VG_FAST_SMALLK ? 0u : 1u) : 0};
}

// what a context can do, copied out of it (adopt_image sets them: fast27_small => fast27_lds => fast27 => k = 27, fastk_small => k != 27,
// pt_index => fast27_small or fastk_small, a table of either kind => neither LDS-filter path)
struct vg_count_caps {
    bool xt_cb, xt_lines;      // context table, grid-16-mer table
    bool fast27, fast27_lds, fast27_small, fastk_small, pt_index;
    bool force_generic;        // VGMI_GENERIC_KERNEL=1
};

enum vg_tail : uint32_t { VG_TAIL_NONE = 0, VG_TAIL_ROWS = 1, VG_TAIL_SEQ = 2 };      // rows_kernel (odd k), seq_kernel (even k)

struct vg_count_plan {
    uint32_t fast;             // vg_fast
    bool clamp;                // xt_clamp_if_due
    bool debit;                // even k: the debit pass in front of the fast kernel
    bool launch_fast;
    uint32_t tail;             // vg_tail
    bool tail_full;            // rows_geometry's grid / a lane per read; false: one workgroup of rows_kernel, seq_kernel's five behind a
                               // fast kernel with the length on the device
    uint64_t row_end, emit_from, row_begin;      // RowParams
    uint32_t tail27;
};

// device_len: the block's length lives in device memory and n_bytes is only a bound -- the path follows from the flags alone, tail27
// names it, and every launch sizes itself there.  Otherwise the split is made here.  Kept as the host form always was:
//   * odd k: a table path clamps even under one row; the fast kernel runs only over complete rows; the tail only where it has ends left
//   * even k: a block under one row (pair of rows) of its fast path is not on that path at all -- no clamp either, which looks like an
//     accident under 768 bytes of a context table and is kept
//   * the table kernels count their rows themselves: RowParams::row_end stays 0 for them
VG_HD vg_count_plan count_plan(const vg_count_caps& f, uint32_t k, uint64_t n_bytes, bool device_len)
{
    const bool odd = k & 1u;
    uint32_t fast = VG_FAST_NONE;
    if (f.force_generic) fast = VG_FAST_NONE;
    else if (f.xt_cb || (odd && f.xt_lines)) fast = VG_FAST_TABLE;
    else if (odd && f.fast27_small) fast = VG_FAST_SMALL27;
    else if (f.fastk_small && f.pt_index) fast = VG_FAST_SMALLK;
    else if (odd && f.fast27) fast = VG_FAST_ROWS27;
    const vg_split s = device_len ? vg_split{0, 0} : vg_row_split(fast, n_bytes);
    if (!device_len && !odd && !s.row_end) fast = VG_FAST_NONE;
    vg_count_plan pl{};
    pl.fast = fast;
    pl.clamp = fast == VG_FAST_TABLE;
    pl.debit = !odd && fast != VG_FAST_NONE;
    pl.launch_fast = fast != VG_FAST_NONE && (device_len || s.row_end);
    pl.tail = !device_len && fast != VG_FAST_NONE && s.emit_from >= n_bytes ? VG_TAIL_NONE : odd ? VG_TAIL_ROWS : VG_TAIL_SEQ;
    pl.tail_full = fast == VG_FAST_NONE || (!odd && !device_len);
    pl.row_end = fast == VG_FAST_TABLE ? 0 : s.row_end;
    pl.emit_from = s.emit_from;
    pl.row_begin = odd ? s.emit_from >> 10 : 0;
    pl.tail27 = device_len ? fast : VG_FAST_NONE;
    return pl;
}

#endif
