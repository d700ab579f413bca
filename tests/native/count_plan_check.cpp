// count_plan_check.cpp -- csrc/vgmi_count_plan.h against a plain model of launch_count as it stood before the plan existed: its four
// decision trees (odd / even k, the block's length on the host / in device memory) written out branch by branch, recording the steps
// instead of launching them.  Stand-alone; meant to run under -fsanitize=address,undefined.
#include <cstdint>
#include <cstdio>

#include "vgmi_count_plan.h"

namespace {
enum Grid : uint32_t { G_NONE, G_ONE, G_FIVE, G_FULL };

struct Steps {
    bool clamp = false, debit = false;
    uint32_t fast = 0;                                        // the fast kernel launched (vg_fast), 0: none
    uint32_t tail = VG_TAIL_NONE, grid = G_NONE;
    uint64_t fast_row_end = 0;                                // RowParams as the fast kernel reads it
    uint64_t debit_emit_from = 0;                             // ... the debit pass
    uint32_t debit_tail27 = 0;
    uint64_t row_end = 0, emit_from = 0, row_begin = 0;       // ... the tail
    uint32_t tail27 = 0;
};

struct P {      // the fields of RowParams the branches write
    uint64_t row_end = 0, emit_from = 0, row_begin = 0;
    uint32_t tail27 = 0;
};

void debit(Steps& s, const P& p) { s.debit = true, s.debit_emit_from = p.emit_from, s.debit_tail27 = p.tail27; }
void fast(Steps& s, const P& p, uint32_t which) { s.fast = which, s.fast_row_end = p.row_end; }
void tail(Steps& s, const P& p, uint32_t which, uint32_t grid)
{
    s.tail = which, s.grid = grid, s.row_end = p.row_end, s.emit_from = p.emit_from, s.row_begin = p.row_begin, s.tail27 = p.tail27;
}

Steps model(const vg_count_caps& c, uint32_t k, uint64_t n_bytes, bool dev)
{
    Steps s;
    P p;
    if (dev && !(k & 1)) {
        if (c.xt_cb && !c.force_generic) {
            s.clamp = true;
            p.tail27 = 2;
            debit(s, p);
            fast(s, p, 2);
            tail(s, p, VG_TAIL_SEQ, G_FIVE);
        } else if (c.fastk_small && c.pt_index && !c.force_generic) {
            p.tail27 = 4;
            debit(s, p);
            fast(s, p, 4);
            tail(s, p, VG_TAIL_SEQ, G_FIVE);
        } else {
            tail(s, p, VG_TAIL_SEQ, G_FULL);
        }
    } else if (dev) {
        if ((c.xt_lines || c.xt_cb) && !c.force_generic) {
            s.clamp = true;
            fast(s, p, 2);
            p.tail27 = 2;
            tail(s, p, VG_TAIL_ROWS, G_ONE);
        } else if ((c.fast27_small || (c.fastk_small && c.pt_index)) && !c.force_generic) {
            fast(s, p, c.fast27_small ? 3 : 4);
            p.tail27 = c.fast27_small ? 3 : 4;
            tail(s, p, VG_TAIL_ROWS, G_ONE);
        } else if (c.fast27 && !c.force_generic) {
            fast(s, p, 1);
            p.tail27 = 1;
            tail(s, p, VG_TAIL_ROWS, G_ONE);
        } else {
            tail(s, p, VG_TAIL_ROWS, G_FULL);
        }
    } else if (k & 1) {
        if ((c.xt_lines || c.xt_cb) && !c.force_generic) {
            const uint64_t rows = n_bytes / 768;
            uint64_t emit_from = 0;
            s.clamp = true;
            if (rows) {
                fast(s, p, 2);
                emit_from = rows * 768 - 1;
            }
            if (emit_from < n_bytes) {
                p.emit_from = emit_from;
                p.row_begin = emit_from >> 10;
                tail(s, p, VG_TAIL_ROWS, G_ONE);
            }
        } else if ((c.fast27_small || (c.fastk_small && c.pt_index)) && !c.force_generic) {
            p.row_end = (n_bytes / 2048) * 2;
            uint64_t emit_from = 0;
            if (p.row_end) {
                fast(s, p, c.fast27_small ? 3 : 4);
                emit_from = p.row_end * 1024 - (c.fast27_small ? 1 : 0);
            }
            if (emit_from < n_bytes) {
                p.emit_from = emit_from;
                p.row_begin = emit_from >> 10;
                tail(s, p, VG_TAIL_ROWS, G_ONE);
            }
        } else if (c.fast27 && !c.force_generic) {
            p.row_end = (n_bytes / 1536) * 2;
            uint64_t emit_from = 0;
            if (p.row_end) {
                fast(s, p, 1);
                emit_from = p.row_end * 768 - 1;
            }
            if (emit_from < n_bytes) {
                p.emit_from = emit_from;
                p.row_begin = emit_from >> 10;
                tail(s, p, VG_TAIL_ROWS, G_ONE);
            }
        } else {
            tail(s, p, VG_TAIL_ROWS, G_FULL);
        }
    } else {
        if (c.xt_cb && !c.force_generic && n_bytes >= 768) {
            const uint64_t rows = n_bytes / 768;
            p.emit_from = rows * 768 - 1;
            s.clamp = true;
            debit(s, p);
            fast(s, p, 2);
            tail(s, p, VG_TAIL_SEQ, G_FULL);
        } else if (c.fastk_small && c.pt_index && !c.force_generic && n_bytes >= 2048) {
            p.row_end = (n_bytes / 2048) * 2;
            p.emit_from = p.row_end * 1024;
            debit(s, p);
            fast(s, p, 4);
            if (p.emit_from < n_bytes) tail(s, p, VG_TAIL_SEQ, G_FULL);
        } else {
            tail(s, p, VG_TAIL_SEQ, G_FULL);
        }
    }
    return s;
}

size_t failures = 0;
void expect(bool ok, const char* what, const vg_count_caps& c, uint32_t k, uint64_t n, bool dev)
{
    if (ok) return;
    if (failures++ < 20)
        std::fprintf(stderr, "MISMATCH %s: cb %d lines %d fast27 %d lds %d small %d fastk %d pt %d generic %d, k %u, n %llu, %s length\n", what, c.xt_cb,
                     c.xt_lines, c.fast27, c.fast27_lds, c.fast27_small, c.fastk_small, c.pt_index, c.force_generic, k, (unsigned long long)n,
                     dev ? "device" : "host");
}

// what adopt_image and the table builders guarantee about a context's flags
bool possible(const vg_count_caps& c, uint32_t k)
{
    if (c.fast27_small && !c.fast27_lds) return false;                          // fast27_small => fast27_lds => fast27
    if (c.fast27_lds && !c.fast27) return false;
    if (c.fast27 && k != 27) return false;                                      // fast27 => k = 27
    if (c.fastk_small && !(k >= 19 && k <= 25)) return false;                   // fastk_small => k = 19 .. 25
    if (c.pt_index && !(c.fast27_small || c.fastk_small)) return false;         // the path table is built for count27s_kernel only
    if (c.xt_cb && c.xt_lines) return false;                                    // one table or the other
    if ((c.xt_cb || c.xt_lines) && (c.fast27_lds || c.fastk_small)) return false;      // a table => no LDS-resident grid filter
    if (c.xt_lines && k != 27) return false;                                    // the grid-16-mer table serves k = 27 only
    return true;
}

// the rows of a fast kernel, from its lanes: a row is 64 lanes of `lane` bytes each, a lane covers the `lane` ends from its first byte + first on
struct Geometry {
    uint64_t lane, rows_per_step;
    int first;
};
const Geometry geometry[5] = {{0, 0, 0}, {12, 2, -1}, {12, 1, -1}, {16, 2, -1}, {16, 2, 0}};
}      // namespace

int main()
{
    const uint64_t sizes[] = {1,    2,    700,  767,  768,  769,  1535,      1536,    1537,    2047,
                              2048, 2049, 3071, 3072, 3073, 4095, 4096,      4097,    6154,    (1u << 20) - 1,
                              1u << 20, (1ull << 32) + 5};
    const uint32_t ks[] = {21, 27, 22, 28};
    size_t n_cases = 0;
    for (uint32_t bits = 0; bits < 256; ++bits) {
        const vg_count_caps c{(bits & 1) != 0,  (bits & 2) != 0,  (bits & 4) != 0,  (bits & 8) != 0,
                              (bits & 16) != 0, (bits & 32) != 0, (bits & 64) != 0, (bits & 128) != 0};
        for (uint32_t k : ks) {
            if (!possible(c, k)) continue;
            for (uint64_t n : sizes)
                for (int dev = 0; dev < 2; ++dev) {
                    const Steps m = model(c, k, n, dev != 0);
                    const vg_count_plan pl = count_plan(c, k, n, dev != 0);
                    ++n_cases;
                    expect(pl.clamp == m.clamp, "clamp", c, k, n, dev);
                    expect(pl.debit == m.debit, "debit", c, k, n, dev);
                    expect((pl.launch_fast ? pl.fast : 0u) == m.fast, "fast kernel", c, k, n, dev);
                    expect(!pl.launch_fast || pl.row_end == m.fast_row_end, "row_end of the fast kernel", c, k, n, dev);
                    expect(!pl.debit || (pl.emit_from == m.debit_emit_from && pl.tail27 == m.debit_tail27), "emit_from / tail27 of the debit pass", c, k, n, dev);
                    expect(pl.tail == m.tail, "tail", c, k, n, dev);
                    if (m.tail != VG_TAIL_NONE) {
                        // the grid: rows_kernel gets one workgroup or rows_geometry's; seq_kernel's launcher gives a lane per read, or five
                        // workgroups where tail27 and the device-side number of reads are set
                        const uint32_t grid = m.tail == VG_TAIL_ROWS ? (pl.tail_full ? G_FULL : G_ONE) : (dev && pl.tail27 ? G_FIVE : G_FULL);
                        expect(grid == m.grid, "grid of the tail", c, k, n, dev);
                        expect(pl.tail_full == (m.grid == G_FULL), "tail_full", c, k, n, dev);
                        expect(pl.row_end == m.row_end && pl.emit_from == m.emit_from && pl.row_begin == m.row_begin && pl.tail27 == m.tail27,
                               "RowParams of the tail", c, k, n, dev);
                    }
                    // the host form and the rule the kernels apply to a length in device memory: the same split wherever the host launches
                    // the fast kernel (the fast kernels count their rows as n / 768, 2 (n / 1536), 2 (n / 2048))
                    if (!dev && pl.launch_fast) {
                        const vg_split d = vg_row_split(count_plan(c, k, n, true).tail27, n);
                        const uint64_t own = pl.fast == VG_FAST_TABLE ? n / 768 : pl.fast == VG_FAST_ROWS27 ? 2 * (n / 1536) : 2 * (n / 2048);
                        expect(d.emit_from == pl.emit_from && d.row_end == own && (pl.fast == VG_FAST_TABLE || pl.row_end == own), "host and device split", c,
                               k, n, dev);
                    }
                }
        }
    }
    // the split against the rows' coverage, lane by lane
    for (uint32_t f = 0; f <= 4; ++f)
        for (uint64_t n : sizes) {
            const vg_split s = vg_row_split(f, n);
            const Geometry& g = geometry[f];
            uint64_t rows = 0, first_uncovered = 0;
            if (f) {
                const uint64_t row_bytes = 64 * g.lane;
                rows = n / (row_bytes * g.rows_per_step) * g.rows_per_step;
                if (rows) {
                    const uint64_t r = rows - 1;      // the last row's lanes, in order: each starts where the one before ended
                    uint64_t next = r * row_bytes + g.first;
                    for (uint64_t lane = 0; lane < 64; ++lane) {
                        if (r * row_bytes + lane * g.lane + g.first != next) ++failures;
                        next += g.lane;
                    }
                    first_uncovered = next;
                    if (rows > 1 && (r - 1) * row_bytes + 63 * g.lane + g.first + g.lane != r * row_bytes + g.first) ++failures;      // rows abut
                }
            }
            if (s.row_end != rows || s.emit_from != first_uncovered || s.emit_from > n) {
                if (failures++ < 20)
                    std::fprintf(stderr, "MISMATCH split: fast %u, n %llu: rows %llu / %llu, emit_from %llu / %llu\n", f, (unsigned long long)n,
                                 (unsigned long long)s.row_end, (unsigned long long)rows, (unsigned long long)s.emit_from, (unsigned long long)first_uncovered);
            }
        }
    if (failures) {
        std::fprintf(stderr, "%zu mismatches\n", failures);
        return 1;
    }
    std::printf("count plan identical to the model: %zu cases\n", n_cases);
    return 0;
}
