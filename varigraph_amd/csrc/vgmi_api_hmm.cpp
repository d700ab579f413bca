// vgmi_api_hmm.cpp -- the HMM on the device (vgmi_hmm_*): emission scores, recursion, posterior, tallies (kernels: vgmi_hmm.hip)
#include "vgmi_ctx.h"

struct vgmi_hmm_part {
    vgmi_ctx* c = nullptr;
    uint8_t* d_obs = nullptr;
    size_t obs_bytes = 0;      // of the block d_obs came as
    uint64_t n_rows = 0;
    uint32_t n_gt = 0;
    // the emission launch's arguments and the block its row arrays and tables live in: vgmi_hmm_part_fix_rows scores rows again
    HmmEmitParams emit{};
    uint8_t* d_small = nullptr;
    size_t small_bytes = 0;
    std::vector<uint32_t> entry_count;      // (host copy: fix_j is checked against it)
    // a part of vgmi_hmm_emissions_select_ploidy, _wide (a genotype list per window): its launch instead, for vgmi_hmm_part_fix_rows_wide and
    // vgmi_hmm_part_fix_rows_ploidy_wide
    bool per_window_lists = false;
    HmmEmitWinParams emit_win{};
    uint32_t wide_words = 0;      // of a _wide call: W words of haplotype bits per entry, and per mask over haplotype ids; 0: packed entries
};

namespace {
// Device working memory of the HMM calls is kept in the context between calls: hipFree waits for every stream of the device --
// other parts', other samples' chains -- so nothing is freed while samples are genotyped.
uint8_t* hmm_block_take(vgmi_ctx* c, size_t bytes, size_t& got)
{
    {
        std::lock_guard<std::mutex> lock(c->hmm_mu);
        size_t best = SIZE_MAX;
        for (size_t i = 0; i < c->hmm_blocks.size(); ++i)
            if (c->hmm_blocks[i].second >= bytes && (best == SIZE_MAX || c->hmm_blocks[i].second < c->hmm_blocks[best].second)) best = i;
        if (best != SIZE_MAX) {
            uint8_t* d = c->hmm_blocks[best].first;
            got = c->hmm_blocks[best].second;
            c->hmm_blocks.erase(c->hmm_blocks.begin() + (ptrdiff_t)best);
            return d;
        }
    }
    uint8_t* d = nullptr;
    got = bytes;
    if (hipMalloc(reinterpret_cast<void**>(&d), bytes) == hipSuccess) return d;
    (void)hipGetLastError();
    std::vector<std::pair<uint8_t*, size_t>> drop;     // the kept ones that are too small make room
    {
        std::lock_guard<std::mutex> lock(c->hmm_mu);
        drop.swap(c->hmm_blocks);
    }
    for (auto& b : drop) (void)hipFree(b.first);
    if (hipMalloc(reinterpret_cast<void**>(&d), bytes) == hipSuccess) return d;
    (void)hipGetLastError();
    return nullptr;
}

void hmm_block_give(vgmi_ctx* c, uint8_t* d, size_t bytes)
{
    if (!d) return;
    std::lock_guard<std::mutex> lock(c->hmm_mu);
    c->hmm_blocks.emplace_back(d, bytes);
}

// one device block carved into pieces: add() hands out 256-aligned offsets, `total` covers the last piece
struct HmmLayout {
    size_t total = 0;
    size_t add(size_t bytes)
    {
        const size_t at = total;
        total = (total + bytes + 255) & ~(size_t)255;
        return at;
    }
};

// One staged call of the HMM: a block of the context's pool laid out by add(), a non-blocking stream of its own (other parts' and
// samples' work on the device is not waited for), copies and launches on it.  The first error sticks and turns every later step into a
// no-op; finish() waits, lets go of the stream and the block and returns that error.  So does the destructor, without waiting.
class HmmCall {
public:
    explicit HmmCall(vgmi_ctx* c) : c_(c) {}
    HmmCall(const HmmCall&) = delete;
    HmmCall& operator=(const HmmCall&) = delete;
    ~HmmCall() { release(); }
    size_t add(size_t bytes) { return lay_.add(bytes); }
    // the device, the block, the stream; `who` names the call in the message
    int begin(const char* who)
    {
        HIPCHK(c_, hipSetDevice(c_->device));
        d_ = hmm_block_take(c_, lay_.total ? lay_.total : 256, bytes_);
        if (!d_) return fail(c_, VGMI_E_NOMEM, std::string(who) + ": not enough device memory");
        note(hipStreamCreateWithFlags(&st_, hipStreamNonBlocking));
        return VGMI_OK;
    }
    template <class T = uint8_t>
    T* at(size_t off) const { return reinterpret_cast<T*>(d_ + off); }
    hipStream_t stream() const { return st_; }
    bool ok() const { return e_ == hipSuccess; }
    void note(hipError_t e) { if (ok()) e_ = e; }
    template <class Launch>
    void run(Launch&& launch) { if (ok()) e_ = launch(); }
    void upload(size_t off, const void* src, size_t bytes) { if (ok() && bytes) e_ = hipMemcpyAsync(d_ + off, src, bytes, hipMemcpyHostToDevice, st_); }
    void zero(size_t off, size_t bytes) { if (ok() && bytes) e_ = hipMemsetAsync(d_ + off, 0, bytes, st_); }
    void download(void* dst, size_t off, size_t bytes) { if (ok() && bytes) e_ = hipMemcpyAsync(dst, d_ + off, bytes, hipMemcpyDeviceToHost, st_); }
    void sync() { if (ok() && st_) e_ = hipStreamSynchronize(st_); }
    // keep_d: where the block goes instead of the pool when all went well (a part keeps its row arrays and tables)
    hipError_t finish(uint8_t** keep_d = nullptr, size_t* keep_bytes = nullptr)
    {
        sync();
        if (ok() && keep_d) {
            *keep_d = d_;
            *keep_bytes = bytes_;
            d_ = nullptr;
        }
        release();
        return e_;
    }

private:
    void release()
    {
        if (st_) (void)hipStreamDestroy(st_);
        st_ = nullptr;
        hmm_block_give(c_, d_, bytes_);
        d_ = nullptr;
    }
    vgmi_ctx* c_;
    HmmLayout lay_;
    uint8_t* d_ = nullptr;
    size_t bytes_ = 0;
    hipStream_t st_ = nullptr;
    hipError_t e_ = hipSuccess;
};

// VGMI_HMM_TIMING=1 for a staged call: upload / kernel / download, milliseconds on stderr (diagnostics)
struct HmmCallTimes {
    bool on;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    explicit HmmCallTimes(bool wanted = true) : on(wanted && getenv("VGMI_HMM_TIMING") != nullptr)
    {
        if (on)
            for (auto& x : ev) (void)hipEventCreate(&x);
    }
    ~HmmCallTimes()
    {
        if (on)
            for (auto& x : ev) (void)hipEventDestroy(x);
    }
    void mark(int i, hipStream_t st) { if (on) (void)hipEventRecord(ev[i], st); }
    // waits for the call; false: the diagnostics are off
    bool times(HmmCall& call, float& up, float& kern, float& down)
    {
        if (!on) return false;
        call.sync();
        up = kern = down = 0;
        if (call.ok()) {
            (void)hipEventElapsedTime(&up, ev[0], ev[1]);
            (void)hipEventElapsedTime(&kern, ev[1], ev[2]);
            (void)hipEventElapsedTime(&down, ev[2], ev[3]);
        }
        return true;
    }
    void report(HmmCall& call, const char* what, uint64_t n_rows, uint32_t bit_len)
    {
        float up, kern, down;
        if (!times(call, up, kern, down)) return;
        fprintf(stderr, "[vgmi] HMM %s call, %u bytes of haplotype bits: %llu rows, upload %.2f ms, kernel %.2f ms, download %.2f ms\n", what, bit_len,
                (unsigned long long)n_rows, up, kern, down);
    }
};

// ---- input checks (`who` names the call in the message) ----
// rows lie inside the uploaded entries and, where rows name windows, in a window that exists
int hmm_check_rows(vgmi_ctx* c, const char* who, uint64_t n_rows, const uint64_t* entry_begin, const uint32_t* entry_count, const uint32_t* row_win = nullptr,
                   uint32_t n_windows = 0)
{
    for (uint64_t r = 0; r < n_rows; ++r)
        if (entry_begin[r] > c->hmm_n_entries || entry_count[r] > c->hmm_n_entries - entry_begin[r] || (row_win && row_win[r] >= n_windows))
            return fail(c, VGMI_E_INVALID, std::string(who) + ": a row outside the entries or the windows");
    return VGMI_OK;
}

// the many-genotype kernel reads keep[p][g] for keep[g][p]: what two genotypes share is symmetric
int hmm_check_keep(vgmi_ctx* c, const char* who, const uint8_t* keep, uint32_t n_windows, uint32_t n_gt)
{
    if (n_gt <= 128) return VGMI_OK;
    for (uint32_t w = 0; w < n_windows; ++w) {
        const uint8_t* m = keep + (size_t)w * n_gt * n_gt;
        for (uint32_t i = 0; i < n_gt; ++i)
            for (uint32_t j = i + 1; j < n_gt; ++j)
                if (m[(size_t)i * n_gt + j] != m[(size_t)j * n_gt + i]) return fail(c, VGMI_E_INVALID, std::string(who) + ": keep matrix not symmetric");
    }
    return VGMI_OK;
}

// beyond 128 genotypes the step table of a whole node lives in LDS, 12 x n_gt x (ploidy + 2) bytes (hmm_recursion_big_kernel) of the 160 KiB a
// workgroup can have: 2 048 genotypes up to ploidy 4, 1 364 at ploidy 8
int hmm_check_lds(vgmi_ctx* c, const char* who, uint32_t n_gt, uint32_t ploidy)
{
    if (n_gt > 128 && (size_t)n_gt * (ploidy + 2) * 12 + 64 > (size_t)160 * 1024)
        return fail(c, VGMI_E_INVALID, std::string(who) + ": more than 128 genotypes of this many haplotypes do not fit the device's local memory");
    return VGMI_OK;
}

// chains, steps and (with fwd_step) rows point inside rows [row_lo, row_hi) and steps [step_lo, step_hi)
int hmm_check_ranges(vgmi_ctx* c, const char* who, const vgmi_hmm_chain* chains, uint32_t n_chains, uint32_t n_windows, const uint32_t* row, uint64_t row_lo,
                     uint64_t row_hi, uint64_t step_lo, uint64_t step_hi, const uint64_t* fwd_step, const uint64_t* bwd_step)
{
    for (uint32_t i = 0; i < n_chains; ++i)
        if (chains[i].keep_index >= n_windows || chains[i].first_step < step_lo || chains[i].first_step + chains[i].n_steps > step_hi)
            return fail(c, VGMI_E_INVALID, std::string(who) + ": a chain points outside its arrays");
    for (uint64_t s = step_lo; s < step_hi; ++s)
        if (row[s] < row_lo || row[s] >= row_hi) return fail(c, VGMI_E_INVALID, std::string(who) + ": a step points outside the emission rows");
    if (fwd_step)
        for (uint64_t i = row_lo; i < row_hi; ++i)
            if (fwd_step[i] < step_lo || fwd_step[i] >= step_hi || bwd_step[i] < step_lo || bwd_step[i] >= step_hi)
                return fail(c, VGMI_E_INVALID, std::string(who) + ": a row points outside the steps");
    return VGMI_OK;
}

// ---- small conversions ----
// pos[2 g], pos[2 g + 1] = pos_a[g], pos_b[g]
std::vector<uint8_t> hmm_pos_pairs(const uint8_t* pos_a, const uint8_t* pos_b, uint32_t n_gt)
{
    std::vector<uint8_t> pos(2 * (size_t)n_gt);
    for (uint32_t g = 0; g < n_gt; ++g) {
        pos[2 * g] = pos_a[g];
        pos[2 * g + 1] = pos_b[g];
    }
    return pos;
}

// a window's haplotypes in 16 ids, whatever n_used; an id is id_bytes wide (1, or 2 for the _wide16 calls)
std::vector<uint8_t> hmm_used16(const void* win_used, size_t n_windows, uint32_t n_used, uint32_t id_bytes = 1)
{
    std::vector<uint8_t> wu16(n_windows * 16 * id_bytes, 0);
    for (size_t w = 0; w < n_windows; ++w) memcpy(&wu16[w * 16 * id_bytes], static_cast<const uint8_t*>(win_used) + w * n_used * id_bytes, (size_t)n_used * id_bytes);
    return wu16;
}

// every id of a window's list is a haplotype of the bit vector
bool hmm_ids_below(const void* win_used, size_t n, uint32_t id_bytes, uint32_t n_ids)
{
    for (size_t i = 0; i < n; ++i)
        if ((id_bytes == 2 ? static_cast<const uint16_t*>(win_used)[i] : static_cast<const uint8_t*>(win_used)[i]) >= n_ids) return false;
    return true;
}

// recursion (+ posterior when gid is given) in one pass over device buffers: alpha / beta leave the device only if `out` asks.
// Every array is indexed by GLOBAL row / step; this call reads and writes rows [row_lo, row_hi) and steps [step_lo, step_hi) only
// (device buffers of that size, the kernels' pointers moved back by the range's start).  It works on a stream of its own and
// touches nothing of the context but its device and error text: calls on parts of the same arrays may run side by side.
int hmm_run(vgmi_ctx* c, uint32_t n_gt, uint32_t ploidy, const uint8_t* keep, uint32_t n_windows, const void* obs, uint64_t row_lo,
            uint64_t row_hi, const uint32_t* row, const uint8_t* restart, const void* pow, uint64_t step_lo, uint64_t step_hi,
            const void* uniform, const vgmi_hmm_chain* chains, uint32_t n_chains, void* out, const uint8_t* gid, const uint8_t* order,
            const uint64_t* fwd_step, const uint64_t* bwd_step, void* prob, uint32_t* winner, const uint8_t* dev_obs = nullptr, const void* freq = nullptr,
            bool by_freq = false)
{
    // dev_obs: the emission rows [row_lo, row_hi) are already on the device (vgmi_hmm_emissions); obs is then not read
    // by_freq: transitions by haplotype frequency (vgmi_hmm_recursion_fre) -- n_windows tables of n_gt x ploidy factors in `freq` take the
    // place of the keep matrices and there are no powers; everything else of the call is the same
    if (!c || (!obs && !dev_obs) || !row || !restart || !uniform || !chains) return VGMI_E_INVALID;
    if (by_freq) {
        if (ploidy < 2 || ploidy > 4) return fail(c, VGMI_E_INVALID, "HMM recursion by haplotype frequency: genotypes of 2..4 haplotypes");
        if (n_gt < 1 || n_gt > 128) return fail(c, VGMI_E_INVALID, "HMM recursion by haplotype frequency: 1..128 genotypes");
        if (!freq || n_windows == 0) return fail(c, VGMI_E_INVALID, "HMM recursion by haplotype frequency: no table of factors");
    } else {
        if (!keep || !pow) return VGMI_E_INVALID;
        if (n_gt < 1 || n_gt > VGMI_HMM_MAX_GT || ploidy < 1 || ploidy > 8) return fail(c, VGMI_E_INVALID, "HMM recursion: 1..2048 genotypes of 1..8 haplotypes");
        if (int rc = hmm_check_lds(c, "HMM recursion", n_gt, ploidy)) return rc;
        if (int rc = hmm_check_keep(c, "HMM recursion", keep, n_windows, n_gt)) return rc;
    }
    if (row_lo > row_hi || step_lo > step_hi) return fail(c, VGMI_E_INVALID, "HMM recursion: an empty-handed range");
    const uint64_t n_rows = row_hi - row_lo, n_steps = step_hi - step_lo;
    if (int rc = hmm_check_ranges(c, "HMM recursion", chains, n_chains, n_windows, row, row_lo, row_hi, step_lo, step_hi, gid ? fwd_step : nullptr, bwd_step)) return rc;
    if (n_steps == 0 || n_chains == 0) return VGMI_OK;
    const uint32_t stride = ploidy + 1;
    // (b_keep: the keep matrices, or the tables of factors in their place)
    const size_t b_keep = by_freq ? (size_t)n_windows * n_gt * ploidy * 16 : (size_t)n_windows * n_gt * n_gt, w_obs = (size_t)n_gt * 16,
                 b_obs = dev_obs ? 0 : (size_t)n_rows * w_obs, b_row = (size_t)n_steps * 4, w_pow = by_freq ? 0 : (size_t)2 * stride * 16, b_pow = (size_t)n_steps * w_pow, b_ch = (size_t)n_chains * sizeof(vgmi_hmm_chain),
                 b_out = (size_t)n_steps * w_obs, b_gid = gid ? (size_t)n_rows * n_gt : 0, b_fs = gid ? (size_t)n_rows * 8 : 0,
                 b_prob = gid ? (size_t)n_rows * 16 : 0, b_win = gid ? (size_t)n_rows * 4 : 0;
    static_assert(sizeof(vgmi_hmm_chain) == sizeof(HmmChain), "chain layout");
    HmmCall call(c);
    const size_t o_keep = call.add(b_keep), o_obs = call.add(b_obs), o_row = call.add(b_row), o_rs = call.add(n_steps), o_pow = call.add(b_pow),
                 o_uni = call.add(16), o_ch = call.add(b_ch), o_out = call.add(b_out), o_gid = call.add(b_gid), o_ord = call.add(b_gid), o_fs = call.add(b_fs),
                 o_bs = call.add(b_fs), o_prob = call.add(b_prob), o_win = call.add(b_win);
    const auto h0 = std::chrono::steady_clock::now();
    if (int rc = call.begin("HMM recursion")) return rc;
    const auto h1 = std::chrono::steady_clock::now();
    hipStream_t st = call.stream();
    // VGMI_HMM_TIMING=1: upload / recursion / posterior + download, milliseconds on stderr (diagnostics)
    const bool timing = getenv("VGMI_HMM_TIMING") != nullptr;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    if (timing)
        for (auto& x : ev) (void)hipEventCreate(&x);
    if (timing) (void)hipEventRecord(ev[0], st);
    call.upload(o_keep, by_freq ? freq : keep, b_keep);
    if (!dev_obs) call.upload(o_obs, static_cast<const uint8_t*>(obs) + row_lo * w_obs, b_obs);
    call.upload(o_row, row + step_lo, b_row);
    call.upload(o_rs, restart + step_lo, n_steps);
    if (!by_freq) call.upload(o_pow, static_cast<const uint8_t*>(pow) + step_lo * w_pow, b_pow);
    call.upload(o_uni, uniform, 16);
    call.upload(o_ch, chains, b_ch);
    if (gid) {
        call.upload(o_gid, gid + row_lo * n_gt, b_gid);
        call.upload(o_ord, order + row_lo * n_gt, b_gid);
        call.upload(o_fs, fwd_step + row_lo, b_fs);
        call.upload(o_bs, bwd_step + row_lo, b_fs);
    }
    const auto h2 = std::chrono::steady_clock::now();
    // where global row / step 0 would lie (the kernels only touch the range)
    auto back = [](uint8_t* p, size_t bytes) { return reinterpret_cast<uint8_t*>(reinterpret_cast<uintptr_t>(p) - bytes); };
    call.run([&] {
        if (by_freq) {
            HmmFreParams F{};
            F.n_gt = n_gt;
            F.ploidy = ploidy;
            F.freq = call.at(o_keep);
            F.obs = back(dev_obs ? const_cast<uint8_t*>(dev_obs) : call.at(o_obs), row_lo * w_obs);
            F.row = reinterpret_cast<const uint32_t*>(back(call.at(o_row), step_lo * 4));
            F.restart = back(call.at(o_rs), step_lo);
            F.uniform = call.at(o_uni);
            F.chains = call.at<const HmmChain>(o_ch);
            F.out = back(call.at(o_out), step_lo * w_obs);
            if (timing) (void)hipEventRecord(ev[1], st);
            const hipError_t e = launch_hmm_recursion_fre(F, n_chains, st);
            if (timing) (void)hipEventRecord(ev[2], st);
            return e;
        }
        HmmParams P{};
        P.n_gt = n_gt;
        P.ploidy = ploidy;
        P.keep = call.at(o_keep);
        P.obs = back(dev_obs ? const_cast<uint8_t*>(dev_obs) : call.at(o_obs), row_lo * w_obs);
        P.row = reinterpret_cast<const uint32_t*>(back(call.at(o_row), step_lo * 4));
        P.restart = back(call.at(o_rs), step_lo);
        P.pow = back(call.at(o_pow), step_lo * w_pow);
        P.uniform = call.at(o_uni);
        P.chains = call.at<const HmmChain>(o_ch);
        P.out = back(call.at(o_out), step_lo * w_obs);
        if (timing) (void)hipEventRecord(ev[1], st);
        const hipError_t e = launch_hmm_recursion(P, n_chains, st);
        if (timing) (void)hipEventRecord(ev[2], st);
        return e;
    });
    if (gid) {
        call.run([&] {
            HmmPostParams Q{};
            Q.n_gt = n_gt;
            Q.row0 = row_lo;
            Q.ab = back(call.at(o_out), step_lo * w_obs);
            Q.fwd_step = reinterpret_cast<const uint64_t*>(back(call.at(o_fs), row_lo * 8));
            Q.bwd_step = reinterpret_cast<const uint64_t*>(back(call.at(o_bs), row_lo * 8));
            Q.gid = back(call.at(o_gid), row_lo * n_gt);
            Q.order = back(call.at(o_ord), row_lo * n_gt);
            Q.prob = back(call.at(o_prob), row_lo * 16);
            Q.winner = reinterpret_cast<uint32_t*>(back(call.at(o_win), row_lo * 4));
            return launch_hmm_posterior(Q, n_rows, st);
        });
        call.download(static_cast<uint8_t*>(prob) + row_lo * 16, o_prob, b_prob);
        call.download(winner + row_lo, o_win, b_win);
    }
    if (out) call.download(static_cast<uint8_t*>(out) + step_lo * w_obs, o_out, b_out);
    if (timing) {
        (void)hipEventRecord(ev[3], st);
        call.sync();
        float a = 0, b = 0, g = 0;
        if (call.ok()) {
            (void)hipEventElapsedTime(&a, ev[0], ev[1]);
            (void)hipEventElapsedTime(&b, ev[1], ev[2]);
            (void)hipEventElapsedTime(&g, ev[2], ev[3]);
        }
        auto ms = [](std::chrono::steady_clock::time_point x, std::chrono::steady_clock::time_point y) { return std::chrono::duration<double, std::milli>(y - x).count(); };
        fprintf(stderr, "[vgmi] HMM on the device%s: %u chains, %llu steps, upload %.1f ms (%.0f MB), recursion %.1f ms, posterior + download %.1f ms; "
                        "host: memory %.1f ms, copies issued in %.1f ms, whole call %.1f ms\n",
                by_freq ? " (by haplotype frequency)" : "", n_chains, (unsigned long long)n_steps, a, (double)(b_keep + b_obs + b_row + b_pow + 2 * b_gid + 2 * b_fs) / 1e6, b, g, ms(h0, h1),
                ms(h1, h2), ms(h0, std::chrono::steady_clock::now()));
        for (auto& x : ev) (void)hipEventDestroy(x);
    }
    HIPCHK(c, call.finish());
    return VGMI_OK;
}

// the entries of vgmi_hmm_entries_upload_wide leave the context (a replaced table, either form)
void hmm_wide_free(vgmi_ctx* c)
{
    if (c->d_hmm_f) (void)hipFree(c->d_hmm_f);
    if (c->d_hmm_bits) (void)hipFree(c->d_hmm_bits);
    c->d_hmm_f = nullptr;
    c->d_hmm_bits = nullptr;
    c->hmm_bit_len = 0;
    c->hmm_words = 0;
}

// a _wide call's width against the upload's: VGMI_E_INVALID for a width no upload can have, VGMI_E_STATE for another form or width
// (ids16: a _wide16 call, whose uploads have 33 to 64 bytes -- so a call of one family on the other's entries differs in width)
int hmm_check_wide(vgmi_ctx* c, const char* who, uint32_t bit_len, bool ids16 = false)
{
    if (ids16 && (bit_len < 33 || bit_len > 64)) return fail(c, VGMI_E_INVALID, std::string(who) + ": 33..64 bytes of haplotype bits");
    if (!ids16 && (bit_len < 1 || bit_len > 32)) return fail(c, VGMI_E_INVALID, std::string(who) + ": 1..32 bytes of haplotype bits");
    if (!c->d_hmm_bits || !c->d_hmm_f || !c->d_hmm_cov || !c->d_hmm_alive)
        return fail(c, VGMI_E_STATE, std::string(who) + (ids16 ? ": upload the entries with vgmi_hmm_entries_upload_wide16 first" : ": upload the entries with vgmi_hmm_entries_upload_wide first"));
    if (bit_len != c->hmm_bit_len) return fail(c, VGMI_E_STATE, std::string(who) + ": the entries were uploaded with another number of bytes of haplotype bits");
    return VGMI_OK;
}

// The storage form an entry point stands for.  A packed call and its _wide namesake are one implementation below; the form says which
// upload it reads, how it is checked, how many words a mask over haplotype ids has, and whether VGMI_HMM_TIMING reports the call (the
// packed calls that never did still do not).
struct HmmForm {
    bool wide;
    uint32_t bit_len;      // the call's (packed: where the call has one)
    bool ids16 = false;    // a _wide16 call: 33 to 64 bytes, a window's drawn haplotypes as 16-bit ids
    // the upload is there and is this form's; `missing`: the packed call's words for none
    int check(vgmi_ctx* c, const char* who, const char* missing, bool need_alive = true) const
    {
        if (wide) return hmm_check_wide(c, who, bit_len, ids16);
        if (!c->d_hmm_entries || !c->d_hmm_cov || (need_alive && !c->d_hmm_alive)) return fail(c, VGMI_E_STATE, std::string(who) + ": " + missing);
        return VGMI_OK;
    }
    uint32_t words(const vgmi_ctx* c) const { return wide ? c->hmm_words : 1u; }
    HmmEntries entries(const vgmi_ctx* c) const { return wide ? HmmEntries{c->d_hmm_f, c->hmm_words, c->d_hmm_bits} : HmmEntries{nullptr, 0u, c->d_hmm_entries}; }
    uint32_t n_ids() const { return 8 * bit_len - 1; }      // the last bit is no haplotype
    uint32_t id_bytes() const { return ids16 ? 2u : 1u; }
};

struct HmmSelect {      // haplotypes selected per window (vgmi_hmm_emissions_select)
    uint32_t n_windows;
    const void* win_used;             // n_windows x n_used ids of the form's width
    const uint64_t* win_top_mask;     // n_windows x the form's words
    const uint32_t* row_win;          // n_rows
};

// What the emission entry points share: the part with its block of scores, and a staged call whose block -- entry_begin | entry_count |
// gt0 | tables | n_kept | flags | the entry point's own arrays -- stays with the part (a fix launch reads the row arrays and tables again).
// Until finish() has handed the part out, the destructor takes it apart.
struct HmmEmitCall {
    vgmi_ctx* c;
    uint64_t n_rows;
    size_t gt0_bytes, tab_bytes;      // per row; of the (ploidy + 1) x 256 terms
    HmmCall call;
    vgmi_hmm_part* part = nullptr;
    size_t o_eb, o_ec, o_g0, o_tab, o_nk, o_fl;
    HmmEmitCall(vgmi_ctx* c_, uint64_t n_rows_, size_t gt0_bytes_, uint32_t ploidy) : c(c_), n_rows(n_rows_), gt0_bytes(gt0_bytes_), tab_bytes((size_t)(ploidy + 1) * 256 * 16), call(c_)
    {
        o_eb = call.add(n_rows * 8);
        o_ec = call.add(n_rows * 4);
        o_g0 = call.add(n_rows * gt0_bytes);
        o_tab = call.add(tab_bytes);
        o_nk = call.add(n_rows * 4);
        o_fl = call.add(n_rows);
    }
    ~HmmEmitCall() { vgmi_hmm_part_free(part); }
    // the part and both blocks, the shared arrays on their way
    int begin(uint32_t n_gt, const uint64_t* entry_begin, const uint32_t* entry_count, const void* gt0, const void* tables)
    {
        HIPCHK(c, hipSetDevice(c->device));
        part = new vgmi_hmm_part;
        part->c = c;
        part->n_rows = n_rows;
        part->n_gt = n_gt;
        part->d_obs = hmm_block_take(c, (size_t)(n_rows ? n_rows : 1) * n_gt * 16, part->obs_bytes);
        if (!part->d_obs) return fail(c, VGMI_E_NOMEM, "HMM emissions: not enough device memory");
        if (int rc = call.begin("HMM emissions")) return rc;
        call.upload(o_eb, entry_begin, n_rows * 8);
        call.upload(o_ec, entry_count, n_rows * 4);
        call.upload(o_g0, gt0, n_rows * gt0_bytes);
        call.upload(o_tab, tables, tab_bytes);
        return VGMI_OK;
    }
    // after the launch (between tm's marks 2 and 3; `what` names the call in the diagnostics): the rows' counts and flags come back, the
    // part goes out
    int finish(HmmCallTimes& tm, const char* what, uint32_t bit_len, const uint32_t* entry_count, uint32_t* n_kept_out, uint8_t* flags_out, vgmi_hmm_part** out)
    {
        if (tm.on) {      // (fetched again below: the figure is the diagnostics')
            call.download(n_kept_out, o_nk, n_rows * 4);
            call.download(flags_out, o_fl, n_rows);
            tm.mark(3, call.stream());
            tm.report(call, what, n_rows, bit_len);
        }
        call.download(n_kept_out, o_nk, n_rows * 4);
        call.download(flags_out, o_fl, n_rows);
        HIPCHK(c, call.finish(&part->d_small, &part->small_bytes));
        part->entry_count.assign(entry_count, entry_count + n_rows);
        *out = part;
        part = nullptr;
        return VGMI_OK;
    }
};

// genotypes as places in a list of haplotypes: the whole panel's one list (sel == nullptr, packed entries only), or a list per window
int hmm_emissions_impl(vgmi_ctx* c, const HmmForm& form, uint32_t n_gt, uint32_t ploidy, uint32_t n_used, const uint8_t* used, const uint8_t* pos, uint64_t top_mask,
                       float ave, double lower, double upper, const void* tables, uint64_t n_rows, const uint64_t* entry_begin, const uint32_t* entry_count,
                       const uint16_t* gt0, uint32_t* n_kept_out, uint8_t* flags_out, vgmi_hmm_part** out, const HmmSelect* sel)
{
    if (!c || !used || !pos || !tables || !out) return VGMI_E_INVALID;
    if (ploidy < 2 || ploidy > 8 || (sel && ploidy != 2)) return fail(c, VGMI_E_INVALID, "HMM emissions: genotypes of 2..8 haplotypes");
    if (n_gt < 1 || n_gt > 128) return fail(c, VGMI_E_INVALID, "HMM emissions: 1..128 genotypes");
    HmmEmitParams P{};
    for (uint32_t g = 0; g < n_gt; ++g) {
        P.pos_a[g] = pos[(size_t)g * ploidy];
        P.pos_b[g] = pos[(size_t)g * ploidy + 1];
        for (uint32_t q = 2; q < ploidy; ++q) P.pos_more[q - 2][g] = pos[(size_t)g * ploidy + q];
        for (uint32_t q = 0; q < ploidy; ++q)
            if (pos[(size_t)g * ploidy + q] >= n_used) return fail(c, VGMI_E_INVALID, "HMM emissions: a genotype names a haplotype outside the list");
    }
    if (n_rows && (!entry_begin || !entry_count || !gt0 || !n_kept_out || !flags_out)) return fail(c, VGMI_E_INVALID, "HMM emissions: rows without their arrays");
    if (n_used < 1 || n_used > 16 || (!form.wide && (form.bit_len < 1 || form.bit_len > 6)))
        return fail(c, VGMI_E_INVALID, "HMM emissions: 1..128 genotypes over 1..16 haplotypes, 1..6 bytes of haplotype bits");
    if (!form.wide && !c->d_hmm_entries) return fail(c, VGMI_E_STATE, "HMM emissions: upload the entries first");
    if (int rc = hmm_check_rows(c, "HMM emissions", n_rows, entry_begin, entry_count, sel ? sel->row_win : nullptr, sel ? sel->n_windows : 0)) return rc;
    *out = nullptr;
    HmmEmitCall ec(c, n_rows, 2, ploidy);
    HmmCall& call = ec.call;
    const size_t n_win = sel ? sel->n_windows : 0, b_mask = n_win * 8 * form.words(c);      // per-window selection: row_win | win_used | win_top_mask
    const size_t o_rw = call.add(sel ? n_rows * 4 : 0), o_wu = call.add(n_win * 16 * form.id_bytes()), o_wm = call.add(b_mask);
    std::vector<uint8_t> wu16;
    if (int rc = ec.begin(n_gt, entry_begin, entry_count, gt0, tables)) return rc;
    HmmCallTimes tm(form.wide);
    tm.mark(0, call.stream());
    P.ent = form.entries(c);
    P.cov = c->d_hmm_cov;
    P.entry_begin = call.at<const uint64_t>(ec.o_eb);
    P.entry_count = call.at<const uint32_t>(ec.o_ec);
    P.gt0 = call.at<const uint16_t>(ec.o_g0);
    P.row_lo = 0;
    P.n_gt = n_gt;
    P.n_used = n_used;
    P.bl8 = 8 * form.bit_len;
    if (!sel) memcpy(P.used, used, n_used);
    P.ploidy = ploidy;
    P.top_mask = top_mask;
    P.ave = ave;
    P.lower = lower;
    P.upper = upper;
    P.tables = call.at(ec.o_tab);
    P.obs = ec.part->d_obs;
    P.n_kept = call.at<uint32_t>(ec.o_nk);
    P.flags = call.at(ec.o_fl);
    if (sel) {
        wu16 = hmm_used16(sel->win_used, n_win, n_used, form.id_bytes());
        call.upload(o_rw, sel->row_win, n_rows * 4);
        call.upload(o_wu, wu16.data(), wu16.size());
        call.upload(o_wm, sel->win_top_mask, b_mask);
        P.row_win = call.at<const uint32_t>(o_rw);
        P.win_used = call.at(o_wu);
        P.win_top_mask = call.at<const unsigned long long>(o_wm);
        P.alive = c->d_hmm_alive;
    }
    tm.mark(1, call.stream());
    call.run([&] { return launch_hmm_emissions(P, n_rows, call.stream()); });
    tm.mark(2, call.stream());
    ec.part->emit = P;
    ec.part->wide_words = P.ent.W;
    return ec.finish(tm, "emission", form.bit_len, entry_count, n_kept_out, flags_out, out);
}

// a genotype LIST per window (vgmi_hmm_emissions_select_ploidy, _wide); `shape` and `who_rows`: the form's words for a refused shape and
// for hmm_check_rows
int hmm_emissions_win_impl(vgmi_ctx* c, const HmmForm& form, const char* shape, const char* who_rows, uint32_t n_gt, uint32_t ploidy, uint32_t n_windows,
                           const uint32_t* win_n_gt, const uint8_t* win_haps, const uint64_t* win_top_mask, float ave, double lower, double upper,
                           const void* tables, uint64_t n_rows, const uint64_t* entry_begin, const uint32_t* entry_count, const uint32_t* row_win,
                           const uint64_t* gt0, uint32_t* n_kept_out, uint8_t* flags_out, vgmi_hmm_part** out)
{
    if (!c || !tables || !out) return VGMI_E_INVALID;
    if (n_gt < 1 || n_gt > 64 || ploidy < 2 || ploidy > 8 || (!form.wide && (form.bit_len < 1 || form.bit_len > 6))) return fail(c, VGMI_E_INVALID, shape);
    if (n_windows < 1 || !win_n_gt || !win_haps || !win_top_mask) return fail(c, VGMI_E_INVALID, "HMM emissions: windows without their genotype lists");
    if (n_rows && (!entry_begin || !entry_count || !row_win || !gt0 || !n_kept_out || !flags_out)) return fail(c, VGMI_E_INVALID, "HMM emissions: rows without their arrays");
    if (int rc = form.check(c, "HMM emissions", "upload the entries first")) return rc;
    const uint32_t W = form.words(c), n_ids = form.n_ids();
    std::vector<uint64_t> used_mask((size_t)n_windows * W, 0);
    for (uint32_t w = 0; w < n_windows; ++w) {
        if (win_n_gt[w] < 1 || win_n_gt[w] > n_gt) return fail(c, VGMI_E_INVALID, "HMM emissions: a window's genotype count outside 1..n_gt");
        for (size_t i = 0; i < (size_t)win_n_gt[w] * ploidy; ++i) {
            const uint32_t hap = win_haps[(size_t)w * n_gt * ploidy + i];
            if (hap >= n_ids) return fail(c, VGMI_E_INVALID, "HMM emissions: a genotype's haplotype outside the haplotype bits");
            used_mask[(size_t)w * W + (hap >> 6)] |= 1ull << (hap & 63u);
        }
        for (uint32_t i = 0; i < W; ++i) {
            const uint64_t hap_bits = n_ids >= 64u * (i + 1u) ? ~0ull : n_ids <= 64u * i ? 0ull : (1ull << (n_ids - 64u * i)) - 1ull;
            if (win_top_mask[(size_t)w * W + i] & ~hap_bits) return fail(c, VGMI_E_INVALID, "HMM emissions: a drawn haplotype outside the haplotype bits");
        }
    }
    if (int rc = hmm_check_rows(c, who_rows, n_rows, entry_begin, entry_count, row_win, n_windows)) return rc;
    *out = nullptr;
    HmmEmitCall ec(c, n_rows, (size_t)8 * W, ploidy);
    HmmCall& call = ec.call;
    const size_t b_haps = (size_t)n_windows * n_gt * ploidy, b_mask = (size_t)n_windows * 8 * W;      // row_win | win_n_gt | win_haps | win_top_mask | win_used_mask
    const size_t o_rw = call.add(n_rows * 4), o_wn = call.add((size_t)n_windows * 4), o_wh = call.add(b_haps), o_wm = call.add(b_mask), o_wu = call.add(b_mask);
    if (int rc = ec.begin(n_gt, entry_begin, entry_count, gt0, tables)) return rc;
    HmmCallTimes tm(form.wide);
    tm.mark(0, call.stream());
    ec.part->per_window_lists = true;
    call.upload(o_rw, row_win, n_rows * 4);
    call.upload(o_wn, win_n_gt, (size_t)n_windows * 4);
    call.upload(o_wh, win_haps, b_haps);
    call.upload(o_wm, win_top_mask, b_mask);
    call.upload(o_wu, used_mask.data(), b_mask);
    HmmEmitWinParams P{};
    P.ent = form.entries(c);
    P.cov = c->d_hmm_cov;
    P.alive = c->d_hmm_alive;
    P.entry_begin = call.at<const uint64_t>(ec.o_eb);
    P.entry_count = call.at<const uint32_t>(ec.o_ec);
    P.row_win = call.at<const uint32_t>(o_rw);
    P.gt0 = call.at<const unsigned long long>(ec.o_g0);
    P.n_gt = n_gt;
    P.ploidy = ploidy;
    P.bl8 = 8 * form.bit_len;
    P.ave = ave;
    P.lower = lower;
    P.upper = upper;
    P.tables = call.at(ec.o_tab);
    P.win_n_gt = call.at<const uint32_t>(o_wn);
    P.win_haps = call.at(o_wh);
    P.win_top_mask = call.at<const unsigned long long>(o_wm);
    P.win_used_mask = call.at<const unsigned long long>(o_wu);
    P.obs = ec.part->d_obs;
    P.n_kept = call.at<uint32_t>(ec.o_nk);
    P.flags = call.at(ec.o_fl);
    P.n_items = n_rows;
    tm.mark(1, call.stream());
    call.run([&] { return launch_hmm_emissions_win(P, call.stream()); });
    tm.mark(2, call.stream());
    ec.part->emit_win = P;
    ec.part->wide_words = P.ent.W;
    return ec.finish(tm, "emission (a genotype list per window)", form.bit_len, entry_count, n_kept_out, flags_out, out);
}

// a part's flagged rows scored again (vgmi_hmm_part_fix_rows*): the part's own launch with the fixes attached -- masks over the places of
// a window's list, or (W words of) haplotype ids
hipError_t hmm_launch_fix(const vgmi_hmm_part& part, uint64_t n, const uint64_t* rows, const uint32_t* off, const uint32_t* j, const uint16_t* mask, hipStream_t st)
{
    HmmEmitParams P = part.emit;
    P.fix_rows = rows;
    P.fix_off = off;
    P.fix_j = j;
    P.fix_mask = mask;
    return launch_hmm_emissions(P, n, st);
}

hipError_t hmm_launch_fix(const vgmi_hmm_part& part, uint64_t n, const uint64_t* rows, const uint32_t* off, const uint32_t* j, const uint64_t* mask, hipStream_t st)
{
    HmmEmitWinParams P = part.emit_win;
    P.n_items = n;
    P.fix_rows = rows;
    P.fix_off = off;
    P.fix_j = j;
    P.fix_mask = reinterpret_cast<const unsigned long long*>(mask);
    return launch_hmm_emissions_win(P, st);
}

// mask_words: how many Masks a fix holds (W for a part of vgmi_hmm_emissions_select_ploidy_wide, else one)
template <class Mask>
int hmm_fix_rows(vgmi_hmm_part* part, uint64_t n, const uint64_t* rows, const uint32_t* fix_off, const uint32_t* fix_j, const Mask* fix_mask, uint32_t mask_words = 1)
{
    vgmi_ctx* c = part->c;
    const uint32_t n_fix = fix_off[n];
    if (n_fix && (!fix_j || !fix_mask)) return VGMI_E_INVALID;
    for (uint64_t r = 0; r < n; ++r) {
        if (rows[r] >= part->n_rows || fix_off[r] > fix_off[r + 1]) return fail(c, VGMI_E_INVALID, "HMM emissions: a fixed row outside the part");
        for (uint32_t i = fix_off[r]; i < fix_off[r + 1]; ++i)
            if (fix_j[i] >= part->entry_count[rows[r]] || (i > fix_off[r] && fix_j[i] <= fix_j[i - 1]))
                return fail(c, VGMI_E_INVALID, "HMM emissions: a row's fixes must name its entries in ascending order");
    }
    HmmCall call(c);
    const size_t o_rows = call.add(n * 8), o_off = call.add((n + 1) * 4), o_j = call.add((size_t)n_fix * 4), o_m = call.add((size_t)n_fix * mask_words * sizeof(Mask));
    if (int rc = call.begin("HMM emissions")) return rc;
    HmmCallTimes tm(part->per_window_lists && part->wide_words);      // (the diagnostics of the calls that have them)
    tm.mark(0, call.stream());
    call.upload(o_rows, rows, n * 8);
    call.upload(o_off, fix_off, (n + 1) * 4);
    call.upload(o_j, fix_j, (size_t)n_fix * 4);
    call.upload(o_m, fix_mask, (size_t)n_fix * mask_words * sizeof(Mask));
    tm.mark(1, call.stream());
    call.run([&] {
        return hmm_launch_fix(*part, n, call.at<const uint64_t>(o_rows), call.at<const uint32_t>(o_off), call.at<const uint32_t>(o_j), call.at<const Mask>(o_m),
                              call.stream());
    });
    tm.mark(2, call.stream());
    tm.mark(3, call.stream());
    tm.report(call, "emission fix", n, part->emit_win.bl8 / 8);
    HIPCHK(c, call.finish());
    return VGMI_OK;
}

// selection support (vgmi_hmm_support, _wide)
int hmm_support_impl(vgmi_ctx* c, const HmmForm& form, uint32_t n_hap, uint32_t n_windows, uint64_t n_rows, const uint64_t* entry_begin, const uint32_t* entry_count,
                     const uint32_t* row_win, uint32_t* support_out)
{
    if (!c || (n_rows && (!entry_begin || !entry_count || !row_win)) || (n_windows && !support_out)) return VGMI_E_INVALID;
    if (!form.wide && (n_hap < 1 || n_hap > 48)) return fail(c, VGMI_E_INVALID, "HMM support: 1..48 haplotypes");
    if (int rc = form.check(c, "HMM support", "upload the entries and the sample's coverage first")) return rc;
    if (form.wide && (n_hap < 1 || n_hap > form.n_ids())) return fail(c, VGMI_E_INVALID, "HMM support: more haplotypes than the haplotype bits hold");
    if (int rc = hmm_check_rows(c, "HMM support", n_rows, entry_begin, entry_count, row_win, n_windows)) return rc;
    if (n_windows == 0) return VGMI_OK;
    const size_t b_sup = (size_t)n_windows * n_hap * 4;
    if (n_rows == 0) {
        memset(support_out, 0, b_sup);
        return VGMI_OK;
    }
    HmmCall call(c);
    const size_t o_beg = call.add(n_rows * 8), o_cnt = call.add(n_rows * 4), o_win = call.add(n_rows * 4), o_sup = call.add(b_sup);
    if (int rc = call.begin("HMM support")) return rc;
    HmmCallTimes tm(form.wide);
    tm.mark(0, call.stream());
    call.upload(o_beg, entry_begin, n_rows * 8);
    call.upload(o_cnt, entry_count, n_rows * 4);
    call.upload(o_win, row_win, n_rows * 4);
    call.zero(o_sup, b_sup);
    tm.mark(1, call.stream());
    call.run([&] {
        return launch_hmm_support(form.entries(c), c->d_hmm_cov, c->d_hmm_alive, call.at<const uint64_t>(o_beg), call.at<const uint32_t>(o_cnt),
                                  call.at<const uint32_t>(o_win), n_rows, n_hap, call.at<uint32_t>(o_sup), call.stream());
    });
    tm.mark(2, call.stream());
    call.download(support_out, o_sup, b_sup);
    tm.mark(3, call.stream());
    tm.report(call, "support", n_rows, form.bit_len);
    HIPCHK(c, call.finish());
    return VGMI_OK;
}

// the calls' tallies with the haplotypes selected per window (vgmi_hmm_tallies_select, _wide); n_ids: the ids a selected haplotype may have
int hmm_tallies_select_impl(vgmi_ctx* c, const HmmForm& form, uint32_t n_ids, uint64_t n_rows, const uint64_t* entry_begin, const uint32_t* entry_count,
                            const uint32_t* row_win, const uint32_t* winner, uint32_t n_gt, const uint8_t* pos_a, const uint8_t* pos_b, uint32_t n_used,
                            uint32_t n_windows, const void* win_used, uint32_t* out, uint8_t* unique_out)
{
    if (!c || (n_rows && (!entry_begin || !entry_count || !row_win || !winner || !out || !unique_out)) || !pos_a || !pos_b || !win_used) return VGMI_E_INVALID;
    if (n_gt < 1 || n_gt > 128 || n_used < 1 || n_used > 16 || n_windows < 1) return fail(c, VGMI_E_INVALID, "HMM tallies: 1..128 genotypes over 1..16 haplotypes");
    if (int rc = form.check(c, "HMM tallies", "upload the entries and the sample's coverage first")) return rc;
    for (uint32_t g = 0; g < n_gt; ++g)
        if (pos_a[g] >= n_used || pos_b[g] >= n_used) return fail(c, VGMI_E_INVALID, "HMM tallies: a genotype names a haplotype outside the list");
    if (!hmm_ids_below(win_used, (size_t)n_windows * n_used, form.id_bytes(), n_ids)) return fail(c, VGMI_E_INVALID, "HMM tallies: a selected haplotype outside the haplotype bits");
    if (int rc = hmm_check_rows(c, "HMM tallies", n_rows, entry_begin, entry_count, row_win, n_windows)) return rc;
    if (n_rows == 0) return VGMI_OK;
    const std::vector<uint8_t> wu16 = hmm_used16(win_used, n_windows, n_used, form.id_bytes()), pos_ab = hmm_pos_pairs(pos_a, pos_b, n_gt);
    HmmCall call(c);
    const size_t o_beg = call.add(n_rows * 8), o_cnt = call.add(n_rows * 4), o_rw = call.add(n_rows * 4), o_win = call.add(n_rows * 4), o_out = call.add(n_rows * 16),
                 o_uni = call.add(n_rows), o_pos = call.add(pos_ab.size()), o_wu = call.add(wu16.size());
    if (int rc = call.begin("HMM tallies")) return rc;
    HmmCallTimes tm(form.wide);
    tm.mark(0, call.stream());
    call.upload(o_beg, entry_begin, n_rows * 8);
    call.upload(o_cnt, entry_count, n_rows * 4);
    call.upload(o_rw, row_win, n_rows * 4);
    call.upload(o_win, winner, n_rows * 4);
    call.upload(o_pos, pos_ab.data(), pos_ab.size());
    call.upload(o_wu, wu16.data(), wu16.size());
    tm.mark(1, call.stream());
    call.run([&] {
        return launch_hmm_tally_select(form.entries(c), c->d_hmm_cov, c->d_hmm_alive, call.at<const uint64_t>(o_beg), call.at<const uint32_t>(o_cnt),
                                       call.at<const uint32_t>(o_rw), call.at<const uint32_t>(o_win), call.at(o_pos), call.at(o_wu), n_gt, n_rows,
                                       call.at<uint32_t>(o_out), call.at(o_uni), call.stream());
    });
    tm.mark(2, call.stream());
    call.download(out, o_out, n_rows * 16);
    call.download(unique_out, o_uni, n_rows);
    tm.mark(3, call.stream());
    tm.report(call, "tally", n_rows, form.bit_len);
    HIPCHK(c, call.finish());
    return VGMI_OK;
}

// the tallies of a polyploid call (vgmi_hmm_tallies_ploidy, _wide)
int hmm_tallies_ploidy_impl(vgmi_ctx* c, const HmmForm& form, uint32_t ploidy, uint32_t n_gt, uint32_t n_windows, const uint32_t* win_n_gt, const uint8_t* win_haps,
                            const uint64_t* win_sel_mask, uint64_t n_rows, const uint64_t* entry_begin, const uint32_t* entry_count, const uint32_t* row_win,
                            const uint32_t* winner, int use_alive, uint32_t* out, uint8_t* unique_out)
{
    if (!c || (n_rows && (!entry_begin || !entry_count || !winner || !out || !unique_out)) || !win_haps || !win_sel_mask) return VGMI_E_INVALID;
    if (ploidy < 2 || ploidy > 4 || n_gt < 1 || n_gt > 128 || n_windows < 1)
        return fail(c, VGMI_E_INVALID, "HMM tallies: 1..128 genotypes of 2..4 haplotypes in at least one window");
    if (int rc = form.check(c, "HMM tallies", "upload the entries and the sample's coverage first", use_alive != 0)) return rc;
    if (win_n_gt)
        for (uint32_t w = 0; w < n_windows; ++w)
            if (win_n_gt[w] > n_gt) return fail(c, VGMI_E_INVALID, "HMM tallies: a window with more genotypes than the lists are wide");
    if (int rc = hmm_check_rows(c, "HMM tallies", n_rows, entry_begin, entry_count, row_win, n_windows)) return rc;
    if (n_rows == 0) return VGMI_OK;
    const size_t b_haps = (size_t)n_windows * n_gt * ploidy, b_out = n_rows * 8 * ploidy, b_mask = (size_t)n_windows * 8 * form.words(c);
    HmmCall call(c);
    const size_t o_beg = call.add(n_rows * 8), o_cnt = call.add(n_rows * 4), o_rw = call.add(row_win ? n_rows * 4 : 0), o_win = call.add(n_rows * 4),
                 o_out = call.add(b_out), o_uni = call.add(n_rows), o_ng = call.add(win_n_gt ? (size_t)n_windows * 4 : 0), o_haps = call.add(b_haps),
                 o_mask = call.add(b_mask);
    if (int rc = call.begin("HMM tallies")) return rc;
    HmmCallTimes tm;
    tm.mark(0, call.stream());
    call.upload(o_beg, entry_begin, n_rows * 8);
    call.upload(o_cnt, entry_count, n_rows * 4);
    if (row_win) call.upload(o_rw, row_win, n_rows * 4);
    call.upload(o_win, winner, n_rows * 4);
    if (win_n_gt) call.upload(o_ng, win_n_gt, (size_t)n_windows * 4);
    call.upload(o_haps, win_haps, b_haps);
    call.upload(o_mask, win_sel_mask, b_mask);
    tm.mark(1, call.stream());
    call.run([&] {
        return launch_hmm_tally_ploidy(form.entries(c), c->d_hmm_cov, use_alive ? c->d_hmm_alive : nullptr, call.at<const uint64_t>(o_beg),
                                       call.at<const uint32_t>(o_cnt), row_win ? call.at<const uint32_t>(o_rw) : nullptr, call.at<const uint32_t>(o_win),
                                       win_n_gt ? call.at<const uint32_t>(o_ng) : nullptr, call.at(o_haps), call.at<const unsigned long long>(o_mask), n_gt, ploidy,
                                       8 * form.bit_len, n_rows, call.at<uint32_t>(o_out), call.at(o_uni), call.stream());
    });
    tm.mark(2, call.stream());
    call.download(out, o_out, b_out);
    call.download(unique_out, o_uni, n_rows);
    tm.mark(3, call.stream());
    if (form.wide) {
        tm.report(call, "tally (polyploid)", n_rows, form.bit_len);
    } else {      // (the packed call's own line, older than report()'s)
        float up, kern, down;
        if (tm.times(call, up, kern, down))
            fprintf(stderr, "[vgmi] HMM tally call: %llu rows of %u haplotypes, upload %.2f ms, kernel %.2f ms, download %.2f ms\n", (unsigned long long)n_rows,
                    ploidy, up, kern, down);
    }
    HIPCHK(c, call.finish());
    return VGMI_OK;
}

}  // namespace

extern "C" {

int vgmi_hmm_entries_upload(vgmi_ctx* c, const uint64_t* entries, size_t n)
{
    if (!c || (n && !entries)) return VGMI_E_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    if (c->d_hmm_entries) (void)hipFree(c->d_hmm_entries);
    if (c->d_hmm_cov) (void)hipFree(c->d_hmm_cov);
    if (c->d_hmm_alive) (void)hipFree(c->d_hmm_alive);
    hmm_wide_free(c);
    c->d_hmm_entries = nullptr;
    c->d_hmm_cov = nullptr;
    c->d_hmm_alive = nullptr;
    c->hmm_n_entries = n;
    if (hipMalloc(reinterpret_cast<void**>(&c->d_hmm_entries), (n ? n : 1) * 8) != hipSuccess ||
        hipMalloc(reinterpret_cast<void**>(&c->d_hmm_cov), n ? n : 1) != hipSuccess ||
        hipMalloc(reinterpret_cast<void**>(&c->d_hmm_alive), n ? n : 1) != hipSuccess)
        return fail(c, VGMI_E_NOMEM, "HMM emissions: not enough device memory for the node-list entries");
    if (n) HIPCHK(c, hipMemcpy(c->d_hmm_entries, entries, n * 8, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemset(c->d_hmm_alive, 1, n ? n : 1));      // a fresh graph: every entry is in its node's list
    return VGMI_OK;
}

// ---- which entries are still in their node's list (src/genotype.cpp:815-818: the forward pass shortens a node's list to the k-mers a
// selected haplotype carries, and ConstructIndex::reset does not restore it).  One byte per entry, next to the entries; all ones after
// vgmi_hmm_entries_upload.  vgmi_hmm_emissions_select clears bytes; the host's lists are uploaded when the host pruned on its own.
int vgmi_hmm_alive_upload(vgmi_ctx* c, const uint8_t* alive, size_t n)
{
    if (!c || (n && !alive)) return VGMI_E_INVALID;
    if (!c->d_hmm_alive || n != c->hmm_n_entries) return fail(c, VGMI_E_STATE, "HMM emissions: upload the entries first");
    HIPCHK(c, hipSetDevice(c->device));
    if (n) HIPCHK(c, hipMemcpy(c->d_hmm_alive, alive, n, hipMemcpyHostToDevice));
    return VGMI_OK;
}

int vgmi_hmm_alive_fetch(vgmi_ctx* c, uint8_t* alive_out, size_t n)
{
    if (!c || (n && !alive_out)) return VGMI_E_INVALID;
    if (!c->d_hmm_alive || n != c->hmm_n_entries) return fail(c, VGMI_E_STATE, "HMM emissions: upload the entries first");
    HIPCHK(c, hipSetDevice(c->device));
    if (n) HIPCHK(c, hipMemcpy(alive_out, c->d_hmm_alive, n, hipMemcpyDeviceToHost));
    return VGMI_OK;
}


// ---- selection support (src/genotype.cpp:500-560, haplotype_selection's sums): support_out[w * n_hap + hap] = sum of c over the alive
// entries of window w's rows with c > 1 and multiplicity <= 1 that haplotype `hap` carries.  The gamma draws stay on the host.
int vgmi_hmm_support(vgmi_ctx* c, uint32_t n_hap, uint32_t n_windows, uint64_t n_rows, const uint64_t* entry_begin, const uint32_t* entry_count,
                     const uint32_t* row_win, uint32_t* support_out)
{
    return hmm_support_impl(c, HmmForm{false, 0}, n_hap, n_windows, n_rows, entry_begin, entry_count, row_win, support_out);
}


int vgmi_hmm_sample_upload(vgmi_ctx* c, const uint8_t* cov_node, size_t n)
{
    if (!c || (n && !cov_node)) return VGMI_E_INVALID;
    if (!c->d_hmm_cov || n != c->hmm_n_entries) return fail(c, VGMI_E_STATE, "HMM emissions: upload the entries first");
    HIPCHK(c, hipSetDevice(c->device));
    if (n) HIPCHK(c, hipMemcpy(c->d_hmm_cov, cov_node, n, hipMemcpyHostToDevice));
    return VGMI_OK;
}

int vgmi_hmm_emissions(vgmi_ctx* c, uint32_t n_gt, uint32_t n_used, const uint8_t* used, const uint8_t* pos_a, const uint8_t* pos_b,
                       uint64_t top_mask, uint32_t bit_len, float ave, double lower, double upper, const void* tables, uint64_t n_rows,
                       const uint64_t* entry_begin, const uint32_t* entry_count, const uint16_t* gt0, uint32_t* n_kept_out,
                       uint8_t* flags_out, vgmi_hmm_part** out)
{
    if (!pos_a || !pos_b || n_gt < 1 || n_gt > 128) return VGMI_E_INVALID;
    return vgmi_hmm_emissions_ploidy(c, n_gt, 2, n_used, used, hmm_pos_pairs(pos_a, pos_b, n_gt).data(), top_mask, bit_len, ave, lower, upper, tables, n_rows,
                                     entry_begin, entry_count, gt0, n_kept_out, flags_out, out);
}


// ... for genotypes of `ploidy` haplotypes (2 .. 8): pos[g * ploidy + q] = the place in `used` of genotype g's q-th haplotype; tables holds
// (ploidy + 1) x 256 terms (geometric for h = 0, Poisson(ave * h) for h = 1 .. ploidy)
int vgmi_hmm_emissions_ploidy(vgmi_ctx* c, uint32_t n_gt, uint32_t ploidy, uint32_t n_used, const uint8_t* used, const uint8_t* pos, uint64_t top_mask,
                              uint32_t bit_len, float ave, double lower, double upper, const void* tables, uint64_t n_rows, const uint64_t* entry_begin,
                              const uint32_t* entry_count, const uint16_t* gt0, uint32_t* n_kept_out, uint8_t* flags_out, vgmi_hmm_part** out)
{
    return hmm_emissions_impl(c, HmmForm{false, bit_len}, n_gt, ploidy, n_used, used, pos, top_mask, ave, lower, upper, tables, n_rows, entry_begin, entry_count, gt0,
                              n_kept_out, flags_out, out, nullptr);
}

// ---- emission scores with the haplotypes selected per window (-n below the panel's haplotypes, a diploid sample) ----------------------
// replaces: hidden_states(..., filter = true) + observable_states (src/genotype.cpp:640-830 with the prune of :673-686 and :815-818,
// :960-1000).  The genotype list has the same shape in every window -- genotype g is the pair (used_w[pos_a[g]], used_w[pos_b[g]]) --
// and row r takes the haplotypes win_used[n_used * row_win[r] ..] and the mask win_top_mask[row_win[r]] of its window.  A row is the
// RANGE [entry_begin, +entry_count) of what remains of its node's list plus the alive bytes; entries a selection does not carry die.
int vgmi_hmm_emissions_select(vgmi_ctx* c, uint32_t n_gt, uint32_t n_used, const uint8_t* pos_a, const uint8_t* pos_b, uint32_t n_windows,
                              const uint8_t* win_used, const uint64_t* win_top_mask, uint32_t bit_len, float ave, double lower, double upper,
                              const void* tables, uint64_t n_rows, const uint64_t* entry_begin, const uint32_t* entry_count, const uint32_t* row_win,
                              const uint16_t* gt0, uint32_t* n_kept_out, uint8_t* flags_out, vgmi_hmm_part** out)
{
    if (!c || !pos_a || !pos_b || !out || n_gt < 1 || n_gt > 128) return VGMI_E_INVALID;
    if (n_windows < 1 || !win_used || !win_top_mask || (n_rows && !row_win)) return fail(c, VGMI_E_INVALID, "HMM emissions: windows without their selections");
    if (n_used < 1 || n_used > 16 || bit_len < 1 || bit_len > 6) return fail(c, VGMI_E_INVALID, "HMM emissions: 1..128 genotypes over 1..16 haplotypes, 1..6 bytes of haplotype bits");
    if (!c->d_hmm_alive) return fail(c, VGMI_E_STATE, "HMM emissions: upload the entries first");
    for (size_t i = 0; i < (size_t)n_windows * n_used; ++i)
        if (win_used[i] >= 8 * bit_len - 1) return fail(c, VGMI_E_INVALID, "HMM emissions: a selected haplotype outside the haplotype bits");
    const HmmSelect sel{n_windows, win_used, win_top_mask, row_win};
    return hmm_emissions_impl(c, HmmForm{false, bit_len}, n_gt, 2, n_used, win_used, hmm_pos_pairs(pos_a, pos_b, n_gt).data(), 0, ave, lower, upper, tables, n_rows,
                              entry_begin, entry_count, gt0, n_kept_out, flags_out, out, &sel);
}


// Rows the emission launch flagged (bit 0: an under-covered multi-copy k-mer that a haplotype of the window carries -- the reference
// then consults the haplotype's sequence, src/genotype.cpp:760-800), scored again with what the host found there: entry fix_j[i] of
// row rows[r] (fix_off[r] <= i < fix_off[r + 1], ascending) loses the haplotypes of fix_mask[i] (bits over the `used` list).  The
// sequences are strings on the host; the products stay on the device.
int vgmi_hmm_part_fix_rows(vgmi_hmm_part* part, uint64_t n, const uint64_t* rows, const uint32_t* fix_off, const uint32_t* fix_j, const uint16_t* fix_mask)
{
    if (!part || (n && (!rows || !fix_off))) return VGMI_E_INVALID;
    if (n == 0) return VGMI_OK;
    if (part->per_window_lists && part->wide_words) return fail(part->c, VGMI_E_STATE, "HMM emissions: this part's fixes are W-word masks over haplotype ids (vgmi_hmm_part_fix_rows_ploidy_wide)");
    if (part->per_window_lists) return fail(part->c, VGMI_E_INVALID, "HMM emissions: this part's fixes are masks over haplotype ids (vgmi_hmm_part_fix_rows_wide)");
    return hmm_fix_rows(part, n, rows, fix_off, fix_j, fix_mask);
}


// ---- emission scores with a genotype LIST per window (-n below the panel's haplotypes, a polyploid sample) -----------------------------
// replaces what vgmi_hmm_emissions_select replaces, for the genotype lists of src/genotype.cpp:846-873: per drawn haplotype the block of
// `ploidy` consecutive haplotypes that holds it, so 1 .. -n genotypes, another number in every window, over haplotypes that were not all
// drawn.  Window w has win_n_gt[w] <= n_gt genotypes, genotype g of it the haplotype ids win_haps[(w * n_gt + g) * ploidy ..]; the prune is
// by win_top_mask[w] (the drawn haplotypes), the scores are over the genotypes' haplotypes; gt0 and the fixes are masks over haplotype ids.
int vgmi_hmm_emissions_select_ploidy(vgmi_ctx* c, uint32_t n_gt, uint32_t ploidy, uint32_t n_windows, const uint32_t* win_n_gt, const uint8_t* win_haps,
                                     const uint64_t* win_top_mask, uint32_t bit_len, float ave, double lower, double upper, const void* tables,
                                     uint64_t n_rows, const uint64_t* entry_begin, const uint32_t* entry_count, const uint32_t* row_win, const uint64_t* gt0,
                                     uint32_t* n_kept_out, uint8_t* flags_out, vgmi_hmm_part** out)
{
    return hmm_emissions_win_impl(c, HmmForm{false, bit_len}, "HMM emissions: 1..64 genotypes of 2..8 haplotypes per window, 1..6 bytes of haplotype bits",
                                  "HMM emissions: a row outside the entries or the windows", n_gt, ploidy, n_windows, win_n_gt, win_haps, win_top_mask, ave, lower, upper,
                                  tables, n_rows, entry_begin, entry_count, row_win, gt0, n_kept_out, flags_out, out);
}

// vgmi_hmm_part_fix_rows for such a part: fix_mask[i] holds the haplotype IDS entry fix_j[i] loses
int vgmi_hmm_part_fix_rows_wide(vgmi_hmm_part* part, uint64_t n, const uint64_t* rows, const uint32_t* fix_off, const uint32_t* fix_j, const uint64_t* fix_mask)
{
    if (!part || (n && (!rows || !fix_off))) return VGMI_E_INVALID;
    if (n == 0) return VGMI_OK;
    if (part->per_window_lists && part->wide_words) return fail(part->c, VGMI_E_STATE, "HMM emissions: this part's fixes are W-word masks over haplotype ids (vgmi_hmm_part_fix_rows_ploidy_wide)");
    if (!part->per_window_lists) return fail(part->c, VGMI_E_INVALID, "HMM emissions: this part's fixes are masks over the `used` list (vgmi_hmm_part_fix_rows)");
    return hmm_fix_rows(part, n, rows, fix_off, fix_j, fix_mask);
}

int vgmi_hmm_part_set_rows(vgmi_hmm_part* part, uint64_t n, const uint64_t* rows, const void* obs_rows)
{
    if (!part || (n && (!rows || !obs_rows))) return VGMI_E_INVALID;
    vgmi_ctx* c = part->c;
    for (uint64_t i = 0; i < n; ++i)
        if (rows[i] >= part->n_rows) return fail(c, VGMI_E_INVALID, "HMM emissions: a row outside the part");
    if (n == 0) return VGMI_OK;
    HmmCall call(c);
    const size_t b_obs = (size_t)n * part->n_gt * 16, o_obs = call.add(b_obs), o_rows = call.add(n * 8);
    if (int rc = call.begin("HMM emissions")) return rc;
    call.upload(o_obs, obs_rows, b_obs);
    call.upload(o_rows, rows, n * 8);
    call.run([&] { return launch_hmm_scatter_rows(part->d_obs, call.at<const uint64_t>(o_rows), call.at(o_obs), part->n_gt, n, call.stream()); });
    HIPCHK(c, call.finish());
    return VGMI_OK;
}


int vgmi_hmm_part_calls(vgmi_hmm_part* part, uint32_t ploidy, const uint8_t* keep, uint32_t n_windows, const uint32_t* row, const uint8_t* restart,
                        const void* pow, uint64_t n_steps, const void* uniform, const vgmi_hmm_chain* chains, uint32_t n_chains, const uint8_t* gid,
                        const uint8_t* order, const uint64_t* fwd_step, const uint64_t* bwd_step, void* prob, uint32_t* winner)
{
    if (!part || !gid || !order || !fwd_step || !bwd_step || !prob || !winner) return VGMI_E_INVALID;
    return hmm_run(part->c, part->n_gt, ploidy, keep, n_windows, nullptr, 0, part->n_rows, row, restart, pow, 0, n_steps, uniform, chains, n_chains,
                   nullptr, gid, order, fwd_step, bwd_step, prob, winner, part->d_obs);
}

// ... under `-m fre`: n_tables tables of the part's n_gt x ploidy factors in place of keep / pow (vgmi_hmm_recursion_fre); the posterior is the same
int vgmi_hmm_part_calls_fre(vgmi_hmm_part* part, uint32_t ploidy, const void* freq, uint32_t n_tables, const uint32_t* row, const uint8_t* restart,
                            uint64_t n_steps, const void* uniform, const vgmi_hmm_chain* chains, uint32_t n_chains, const uint8_t* gid, const uint8_t* order,
                            const uint64_t* fwd_step, const uint64_t* bwd_step, void* prob, uint32_t* winner)
{
    if (!part || !gid || !order || !fwd_step || !bwd_step || !prob || !winner) return VGMI_E_INVALID;
    return hmm_run(part->c, part->n_gt, ploidy, nullptr, n_tables, nullptr, 0, part->n_rows, row, restart, nullptr, 0, n_steps, uniform, chains, n_chains, nullptr,
                   gid, order, fwd_step, bwd_step, prob, winner, part->d_obs, freq, true);
}

// ---- a part's recursion inputs kept on the device (round 5).  Everything hmm_run uploads but the emission scores -- keep matrix, step
// tables (pow), rows, restarts, chains, genotype strings' ids and order, the rows' steps: 230 MB per chr20-scale sample -- is a
// function of the graph and the options, not of the sample: a plan holds it on the device, made once, used by every sample (and every
// context of the device: the block is plain device memory, not a context's pool).
struct vgmi_hmm_plan {
    int device = 0;
    uint8_t* d = nullptr;
    uint32_t n_gt = 0, ploidy = 0, n_chains = 0;
    uint64_t n_rows = 0, n_steps = 0;
    size_t o_keep = 0, o_row = 0, o_rs = 0, o_pow = 0, o_uni = 0, o_ch = 0, o_gid = 0, o_ord = 0, o_fs = 0, o_bs = 0, bytes = 0;
};

int vgmi_hmm_plan_create(vgmi_ctx* c, uint32_t n_gt, uint32_t ploidy, const uint8_t* keep, uint32_t n_windows, uint64_t n_rows, const uint32_t* row,
                         const uint8_t* restart, const void* pow, uint64_t n_steps, const void* uniform, const vgmi_hmm_chain* chains, uint32_t n_chains,
                         const uint8_t* gid, const uint8_t* order, const uint64_t* fwd_step, const uint64_t* bwd_step, vgmi_hmm_plan** out)
{
    if (!c || !out) return VGMI_E_INVALID;
    *out = nullptr;
    if (!keep || !row || !restart || !pow || !uniform || !chains || !gid || !order || !fwd_step || !bwd_step) return VGMI_E_INVALID;
    if (n_gt < 1 || n_gt > VGMI_HMM_MAX_GT || ploidy < 1 || ploidy > 8) return fail(c, VGMI_E_INVALID, "HMM plan: 1..2048 genotypes of 1..8 haplotypes");
    if (int rc = hmm_check_lds(c, "HMM plan", n_gt, ploidy)) return rc;
    if (int rc = hmm_check_keep(c, "HMM plan", keep, n_windows, n_gt)) return rc;
    if (n_steps == 0 || n_chains == 0 || n_rows == 0) return fail(c, VGMI_E_INVALID, "HMM plan: nothing to plan");
    if (int rc = hmm_check_ranges(c, "HMM plan", chains, n_chains, n_windows, row, 0, n_rows, 0, n_steps, fwd_step, bwd_step)) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    auto* pl = new vgmi_hmm_plan;
    pl->device = c->device;
    pl->n_gt = n_gt;
    pl->ploidy = ploidy;
    pl->n_chains = n_chains;
    pl->n_rows = n_rows;
    pl->n_steps = n_steps;
    const uint32_t stride = ploidy + 1;
    const size_t b_keep = (size_t)n_windows * n_gt * n_gt, b_row = (size_t)n_steps * 4, w_pow = (size_t)2 * stride * 16, b_pow = (size_t)n_steps * w_pow,
                 b_ch = (size_t)n_chains * sizeof(vgmi_hmm_chain), b_gid = (size_t)n_rows * n_gt, b_fs = (size_t)n_rows * 8;
    HmmLayout lay;
    pl->o_keep = lay.add(b_keep);
    pl->o_row = lay.add(b_row);
    pl->o_rs = lay.add(n_steps);
    pl->o_pow = lay.add(b_pow);
    pl->o_uni = lay.add(16);
    pl->o_ch = lay.add(b_ch);
    pl->o_gid = lay.add(b_gid);
    pl->o_ord = lay.add(b_gid);
    pl->o_fs = lay.add(b_fs);
    pl->o_bs = lay.add(b_fs);
    pl->bytes = lay.total;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&pl->d), pl->bytes);
    if (e != hipSuccess) {
        delete pl;
        (void)hipGetLastError();
        return fail(c, VGMI_E_NOMEM, "HMM plan: not enough device memory");
    }
    auto put = [&](size_t off, const void* src, size_t bytes) {
        if (e == hipSuccess) e = hipMemcpy(pl->d + off, src, bytes, hipMemcpyHostToDevice);
    };
    put(pl->o_keep, keep, b_keep);
    put(pl->o_row, row, b_row);
    put(pl->o_rs, restart, n_steps);
    put(pl->o_pow, pow, b_pow);
    put(pl->o_uni, uniform, 16);
    put(pl->o_ch, chains, b_ch);
    put(pl->o_gid, gid, b_gid);
    put(pl->o_ord, order, b_gid);
    put(pl->o_fs, fwd_step, b_fs);
    put(pl->o_bs, bwd_step, b_fs);
    if (e != hipSuccess) {
        (void)hipFree(pl->d);
        delete pl;
        HIPCHK(c, e);
    }
    *out = pl;
    return VGMI_OK;
}


void vgmi_hmm_plan_free(vgmi_hmm_plan* pl)
{
    if (!pl) return;
    if (pl->d && hipSetDevice(pl->device) == hipSuccess) (void)hipFree(pl->d);
    delete pl;
}

// recursion and posterior of a part on the inputs of a plan and the part's own emission scores: what comes back is the calls
int vgmi_hmm_part_calls_plan(vgmi_hmm_part* part, const vgmi_hmm_plan* pl, void* prob, uint32_t* winner)
{
    if (!part || !pl || !prob || !winner) return VGMI_E_INVALID;
    vgmi_ctx* c = part->c;
    if (pl->device != c->device || pl->n_gt != part->n_gt || pl->n_rows != part->n_rows) return fail(c, VGMI_E_INVALID, "HMM plan: made for another part");
    const size_t w_obs = (size_t)pl->n_gt * 16, b_prob = (size_t)pl->n_rows * 16, b_win = (size_t)pl->n_rows * 4;
    HmmCall call(c);
    const size_t o_out = call.add((size_t)pl->n_steps * w_obs), o_prob = call.add(b_prob), o_win = call.add(b_win);
    if (int rc = call.begin("HMM recursion")) return rc;
    call.run([&] {
        HmmParams P{};
        P.n_gt = pl->n_gt;
        P.ploidy = pl->ploidy;
        P.keep = pl->d + pl->o_keep;
        P.obs = part->d_obs;
        P.row = reinterpret_cast<const uint32_t*>(pl->d + pl->o_row);
        P.restart = pl->d + pl->o_rs;
        P.pow = pl->d + pl->o_pow;
        P.uniform = pl->d + pl->o_uni;
        P.chains = reinterpret_cast<const HmmChain*>(pl->d + pl->o_ch);
        P.out = call.at(o_out);
        return launch_hmm_recursion(P, pl->n_chains, call.stream());
    });
    call.run([&] {
        HmmPostParams Q{};
        Q.n_gt = pl->n_gt;
        Q.row0 = 0;
        Q.ab = call.at(o_out);
        Q.fwd_step = reinterpret_cast<const uint64_t*>(pl->d + pl->o_fs);
        Q.bwd_step = reinterpret_cast<const uint64_t*>(pl->d + pl->o_bs);
        Q.gid = pl->d + pl->o_gid;
        Q.order = pl->d + pl->o_ord;
        Q.prob = call.at(o_prob);
        Q.winner = call.at<uint32_t>(o_win);
        return launch_hmm_posterior(Q, pl->n_rows, call.stream());
    });
    call.download(prob, o_prob, b_prob);
    call.download(winner, o_win, b_win);
    HIPCHK(c, call.finish());
    return VGMI_OK;
}

int vgmi_hmm_tallies(vgmi_ctx* c, uint64_t n_rows, const uint64_t* entry_begin, const uint32_t* entry_count, const uint32_t* winner, uint32_t n_gt,
                     const uint8_t* hap_ab, uint32_t n_hap, uint64_t sel_mask, uint32_t* out, uint8_t* unique_out)
{
    if (!c || (n_rows && (!entry_begin || !entry_count || !winner || !hap_ab || !out || !unique_out)) || n_gt > 128) return VGMI_E_INVALID;
    if (!c->d_hmm_entries || !c->d_hmm_cov) return fail(c, VGMI_E_STATE, "HMM tallies: upload the entries and the sample's coverage first");
    if (n_rows == 0) return VGMI_OK;
    if (int rc = hmm_check_rows(c, "HMM tallies", n_rows, entry_begin, entry_count)) return rc;
    HmmCall call(c);
    const size_t o_beg = call.add(n_rows * 8), o_cnt = call.add(n_rows * 4), o_win = call.add(n_rows * 4), o_out = call.add(n_rows * 16), o_uni = call.add(n_rows),
                 o_hap = call.add(2 * (size_t)n_gt);
    if (int rc = call.begin("HMM tallies")) return rc;
    call.upload(o_beg, entry_begin, n_rows * 8);
    call.upload(o_cnt, entry_count, n_rows * 4);
    call.upload(o_win, winner, n_rows * 4);
    call.upload(o_hap, hap_ab, 2 * (size_t)n_gt);
    call.run([&] {
        return launch_hmm_tally(c->d_hmm_entries, c->d_hmm_cov, call.at<const uint64_t>(o_beg), call.at<const uint32_t>(o_cnt), call.at<const uint32_t>(o_win),
                                call.at(o_hap), n_gt, n_hap, sel_mask, n_rows, call.at<uint32_t>(o_out), call.at(o_uni), call.stream());
    });
    call.download(out, o_out, n_rows * 16);
    call.download(unique_out, o_uni, n_rows);
    HIPCHK(c, call.finish());
    return VGMI_OK;
}


// ---- the calls' tallies with the haplotypes selected per window (src/genotype.cpp:1387-1414 on the pruned lists): the called genotype
// winner[i] of a row of window w is the pair (win_used[n_used w + pos_a[g]], win_used[n_used w + pos_b[g]]); only alive entries count,
// for the haplotypes' k-mers and for the count of single-copy k-mers alike.
int vgmi_hmm_tallies_select(vgmi_ctx* c, uint64_t n_rows, const uint64_t* entry_begin, const uint32_t* entry_count, const uint32_t* row_win,
                            const uint32_t* winner, uint32_t n_gt, const uint8_t* pos_a, const uint8_t* pos_b, uint32_t n_used, uint32_t n_windows,
                            const uint8_t* win_used, uint32_t* out, uint8_t* unique_out)
{
    return hmm_tallies_select_impl(c, HmmForm{false, 0}, 48, n_rows, entry_begin, entry_count, row_win, winner, n_gt, pos_a, pos_b, n_used, n_windows, win_used, out,
                                   unique_out);
}


// ---- the tallies of a POLYPLOID call (ploidy 3, 4; pairs are taken too): the called genotype winner[i] of a row of window w is the `ploidy`
// ids win_haps[(w * n_gt + g) * ploidy ..] -- the lists the emission launches of such a sample take, the whole panel's being one window
// (row_win == NULL) without alive bytes (use_alive == 0: no list was ever pruned).
int vgmi_hmm_tallies_ploidy(vgmi_ctx* c, uint32_t ploidy, uint32_t n_gt, uint32_t n_windows, const uint32_t* win_n_gt, const uint8_t* win_haps,
                            const uint64_t* win_sel_mask, uint64_t n_rows, const uint64_t* entry_begin, const uint32_t* entry_count, const uint32_t* row_win,
                            const uint32_t* winner, int use_alive, uint32_t* out, uint8_t* unique_out)
{
    return hmm_tallies_ploidy_impl(c, HmmForm{false, 0}, ploidy, n_gt, n_windows, win_n_gt, win_haps, win_sel_mask, n_rows, entry_begin, entry_count, row_win, winner,
                                   use_alive, out, unique_out);
}


// ---- a diploid sample over a panel of 48 to 254 haplotypes (vgmi.h): the entries as a multiplicity byte and W words of haplotype bits ----
namespace {
// vgmi_hmm_entries_reserve_wide (1 to 32 bytes) and _wide16 (33 to 64): one table in the context, whichever call made it
int hmm_entries_reserve_impl(vgmi_ctx* c, size_t n, uint32_t bit_len, bool ids16)
{
    if (!c) return VGMI_E_INVALID;
    if (ids16 && (bit_len < 33 || bit_len > 64)) return fail(c, VGMI_E_INVALID, "HMM entries: 33..64 bytes of haplotype bits");
    if (!ids16 && (bit_len < 1 || bit_len > 32)) return fail(c, VGMI_E_INVALID, "HMM entries: 1..32 bytes of haplotype bits");
    HIPCHK(c, hipSetDevice(c->device));
    if (c->d_hmm_entries) (void)hipFree(c->d_hmm_entries);
    if (c->d_hmm_cov) (void)hipFree(c->d_hmm_cov);
    if (c->d_hmm_alive) (void)hipFree(c->d_hmm_alive);
    hmm_wide_free(c);
    c->d_hmm_entries = nullptr;
    c->d_hmm_cov = nullptr;
    c->d_hmm_alive = nullptr;
    c->hmm_n_entries = n;
    const uint32_t W = bit_len <= 8 ? 1u : bit_len <= 16 ? 2u : bit_len <= 32 ? 4u : 8u;
    if (hipMalloc(reinterpret_cast<void**>(&c->d_hmm_f), n ? n : 1) != hipSuccess ||
        hipMalloc(reinterpret_cast<void**>(&c->d_hmm_bits), (n ? n : 1) * 8 * W) != hipSuccess ||
        hipMalloc(reinterpret_cast<void**>(&c->d_hmm_cov), n ? n : 1) != hipSuccess ||
        hipMalloc(reinterpret_cast<void**>(&c->d_hmm_alive), n ? n : 1) != hipSuccess) {
        (void)hipGetLastError();
        if (c->d_hmm_cov) (void)hipFree(c->d_hmm_cov);
        if (c->d_hmm_alive) (void)hipFree(c->d_hmm_alive);
        c->d_hmm_cov = nullptr;
        c->d_hmm_alive = nullptr;
        hmm_wide_free(c);
        c->hmm_n_entries = 0;
        return fail(c, VGMI_E_NOMEM, "HMM emissions: not enough device memory for the node-list entries");
    }
    c->hmm_bit_len = bit_len;
    c->hmm_words = W;
    HIPCHK(c, hipMemset(c->d_hmm_bits, 0, (n ? n : 1) * 8 * W));
    HIPCHK(c, hipMemset(c->d_hmm_f, 0, n ? n : 1));
    HIPCHK(c, hipMemset(c->d_hmm_alive, 1, n ? n : 1));      // a fresh graph: every entry is in its node's list
    return VGMI_OK;
}

// the _wide and _wide16 emission entry points: win_used holds ids of the form's width
int hmm_emissions_select_wide_impl(vgmi_ctx* c, const HmmForm& form, uint32_t n_gt, uint32_t n_used, const uint8_t* pos_a, const uint8_t* pos_b, uint32_t n_windows,
                                   const void* win_used, const uint64_t* win_top_mask, float ave, double lower, double upper, const void* tables, uint64_t n_rows,
                                   const uint64_t* entry_begin, const uint32_t* entry_count, const uint32_t* row_win, const uint16_t* gt0, uint32_t* n_kept_out,
                                   uint8_t* flags_out, vgmi_hmm_part** out)
{
    if (!c || !pos_a || !pos_b || !tables || !out) return VGMI_E_INVALID;
    if (n_gt < 1 || n_gt > 128 || n_used < 1 || n_used > 16) return fail(c, VGMI_E_INVALID, "HMM emissions: 1..128 genotypes over 1..16 haplotypes");
    if (n_windows < 1 || !win_used || !win_top_mask || (n_rows && !row_win)) return fail(c, VGMI_E_INVALID, "HMM emissions: windows without their selections");
    if (n_rows && (!entry_begin || !entry_count || !gt0 || !n_kept_out || !flags_out)) return fail(c, VGMI_E_INVALID, "HMM emissions: rows without their arrays");
    if (int rc = form.check(c, "HMM emissions", "")) return rc;
    if (!hmm_ids_below(win_used, (size_t)n_windows * n_used, form.id_bytes(), form.n_ids()))
        return fail(c, VGMI_E_INVALID, "HMM emissions: a selected haplotype outside the haplotype bits");
    const HmmSelect sel{n_windows, win_used, win_top_mask, row_win};
    return hmm_emissions_impl(c, form, n_gt, 2, n_used, static_cast<const uint8_t*>(win_used), hmm_pos_pairs(pos_a, pos_b, n_gt).data(), 0, ave, lower, upper, tables,
                              n_rows, entry_begin, entry_count, gt0, n_kept_out, flags_out, out, &sel);
}
// vgmi_hmm_entries_fill_wide and _wide16: each fills the table its own reserve made
int hmm_entries_fill_impl(vgmi_ctx* c, size_t first, size_t n, const uint8_t* f, const uint8_t* bits, bool ids16)
{
    if (!c || (n && (!f || !bits))) return VGMI_E_INVALID;
    if (!c->d_hmm_bits || !c->d_hmm_f || (c->hmm_words == 8) != ids16) return fail(c, VGMI_E_STATE, "HMM entries: reserve the entries first");
    if (first > c->hmm_n_entries || n > c->hmm_n_entries - first) return fail(c, VGMI_E_INVALID, "HMM entries: a range outside the reserved entries");
    HIPCHK(c, hipSetDevice(c->device));
    const uint32_t W = c->hmm_words, bl = c->hmm_bit_len;
    constexpr size_t kChunk = (size_t)1 << 20;      // entries per staged copy
    std::vector<uint64_t> words;
    for (size_t a = 0; a < n; a += kChunk) {
        const size_t m = std::min(kChunk, n - a);
        words.assign(m * W, 0);
        for (size_t j = 0; j < m; ++j) memcpy(&words[j * W], bits + (a + j) * bl, bl);      // (little-endian host: byte i of the vector is byte i of the words)
        HIPCHK(c, hipMemcpy(c->d_hmm_bits + (first + a) * W, words.data(), m * W * 8, hipMemcpyHostToDevice));
    }
    if (n) HIPCHK(c, hipMemcpy(c->d_hmm_f + first, f, n, hipMemcpyHostToDevice));
    return VGMI_OK;
}
}  // namespace

int vgmi_hmm_entries_reserve_wide(vgmi_ctx* c, size_t n, uint32_t bit_len) { return hmm_entries_reserve_impl(c, n, bit_len, false); }

int vgmi_hmm_entries_fill_wide(vgmi_ctx* c, size_t first, size_t n, const uint8_t* f, const uint8_t* bits) { return hmm_entries_fill_impl(c, first, n, f, bits, false); }

int vgmi_hmm_entries_upload_wide(vgmi_ctx* c, const uint8_t* f, const uint8_t* bits, size_t n, uint32_t bit_len)
{
    if (!c || (n && (!f || !bits))) return VGMI_E_INVALID;
    if (int rc = vgmi_hmm_entries_reserve_wide(c, n, bit_len)) return rc;
    return vgmi_hmm_entries_fill_wide(c, 0, n, f, bits);
}

int vgmi_hmm_support_wide(vgmi_ctx* c, uint32_t bit_len, uint32_t n_hap, uint32_t n_windows, uint64_t n_rows, const uint64_t* entry_begin,
                          const uint32_t* entry_count, const uint32_t* row_win, uint32_t* support_out)
{
    return hmm_support_impl(c, HmmForm{true, bit_len}, n_hap, n_windows, n_rows, entry_begin, entry_count, row_win, support_out);
}

int vgmi_hmm_emissions_select_wide(vgmi_ctx* c, uint32_t n_gt, uint32_t n_used, const uint8_t* pos_a, const uint8_t* pos_b, uint32_t n_windows,
                                   const uint8_t* win_used, const uint64_t* win_top_mask, uint32_t bit_len, float ave, double lower, double upper,
                                   const void* tables, uint64_t n_rows, const uint64_t* entry_begin, const uint32_t* entry_count, const uint32_t* row_win,
                                   const uint16_t* gt0, uint32_t* n_kept_out, uint8_t* flags_out, vgmi_hmm_part** out)
{
    return hmm_emissions_select_wide_impl(c, HmmForm{true, bit_len}, n_gt, n_used, pos_a, pos_b, n_windows, win_used, win_top_mask, ave, lower, upper, tables, n_rows,
                                          entry_begin, entry_count, row_win, gt0, n_kept_out, flags_out, out);
}

int vgmi_hmm_tallies_select_wide(vgmi_ctx* c, uint32_t bit_len, uint64_t n_rows, const uint64_t* entry_begin, const uint32_t* entry_count,
                                 const uint32_t* row_win, const uint32_t* winner, uint32_t n_gt, const uint8_t* pos_a, const uint8_t* pos_b, uint32_t n_used,
                                 uint32_t n_windows, const uint8_t* win_used, uint32_t* out, uint8_t* unique_out)
{
    const HmmForm form{true, bit_len};
    return hmm_tallies_select_impl(c, form, form.n_ids(), n_rows, entry_begin, entry_count, row_win, winner, n_gt, pos_a, pos_b, n_used, n_windows, win_used, out,
                                   unique_out);
}

// ---- a diploid sample over a panel of 255 to 511 haplotypes (vgmi.h): 33 to 64 bytes of haplotype bits in eight words per entry, the
// drawn haplotypes of a window as 16-bit ids.  The table is the context's one wide table: either upload replaces the other's arrays.
int vgmi_hmm_entries_reserve_wide16(vgmi_ctx* c, size_t n, uint32_t bit_len) { return hmm_entries_reserve_impl(c, n, bit_len, true); }

int vgmi_hmm_entries_fill_wide16(vgmi_ctx* c, size_t first, size_t n, const uint8_t* f, const uint8_t* bits) { return hmm_entries_fill_impl(c, first, n, f, bits, true); }

int vgmi_hmm_entries_upload_wide16(vgmi_ctx* c, const uint8_t* f, const uint8_t* bits, size_t n, uint32_t bit_len)
{
    if (!c || (n && (!f || !bits))) return VGMI_E_INVALID;
    if (int rc = vgmi_hmm_entries_reserve_wide16(c, n, bit_len)) return rc;
    return vgmi_hmm_entries_fill_wide16(c, 0, n, f, bits);
}

int vgmi_hmm_support_wide16(vgmi_ctx* c, uint32_t bit_len, uint32_t n_hap, uint32_t n_windows, uint64_t n_rows, const uint64_t* entry_begin,
                            const uint32_t* entry_count, const uint32_t* row_win, uint32_t* support_out)
{
    return hmm_support_impl(c, HmmForm{true, bit_len, true}, n_hap, n_windows, n_rows, entry_begin, entry_count, row_win, support_out);
}

int vgmi_hmm_emissions_select_wide16(vgmi_ctx* c, uint32_t n_gt, uint32_t n_used, const uint8_t* pos_a, const uint8_t* pos_b, uint32_t n_windows,
                                     const uint16_t* win_used, const uint64_t* win_top_mask, uint32_t bit_len, float ave, double lower, double upper,
                                     const void* tables, uint64_t n_rows, const uint64_t* entry_begin, const uint32_t* entry_count, const uint32_t* row_win,
                                     const uint16_t* gt0, uint32_t* n_kept_out, uint8_t* flags_out, vgmi_hmm_part** out)
{
    return hmm_emissions_select_wide_impl(c, HmmForm{true, bit_len, true}, n_gt, n_used, pos_a, pos_b, n_windows, win_used, win_top_mask, ave, lower, upper, tables,
                                          n_rows, entry_begin, entry_count, row_win, gt0, n_kept_out, flags_out, out);
}

int vgmi_hmm_tallies_select_wide16(vgmi_ctx* c, uint32_t bit_len, uint64_t n_rows, const uint64_t* entry_begin, const uint32_t* entry_count,
                                   const uint32_t* row_win, const uint32_t* winner, uint32_t n_gt, const uint8_t* pos_a, const uint8_t* pos_b, uint32_t n_used,
                                   uint32_t n_windows, const uint16_t* win_used, uint32_t* out, uint8_t* unique_out)
{
    const HmmForm form{true, bit_len, true};
    return hmm_tallies_select_impl(c, form, form.n_ids(), n_rows, entry_begin, entry_count, row_win, winner, n_gt, pos_a, pos_b, n_used, n_windows, win_used, out,
                                   unique_out);
}

// ---- a POLYPLOID sample over such a panel (vgmi.h): vgmi_hmm_emissions_select_ploidy and vgmi_hmm_tallies_ploidy with every mask over
// haplotype ids W words wide
int vgmi_hmm_emissions_select_ploidy_wide(vgmi_ctx* c, uint32_t n_gt, uint32_t ploidy, uint32_t n_windows, const uint32_t* win_n_gt, const uint8_t* win_haps,
                                          const uint64_t* win_top_mask, uint32_t bit_len, float ave, double lower, double upper, const void* tables,
                                          uint64_t n_rows, const uint64_t* entry_begin, const uint32_t* entry_count, const uint32_t* row_win, const uint64_t* gt0,
                                          uint32_t* n_kept_out, uint8_t* flags_out, vgmi_hmm_part** out)
{
    return hmm_emissions_win_impl(c, HmmForm{true, bit_len}, "HMM emissions: 1..64 genotypes of 2..8 haplotypes per window", "HMM emissions", n_gt, ploidy, n_windows,
                                  win_n_gt, win_haps, win_top_mask, ave, lower, upper, tables, n_rows, entry_begin, entry_count, row_win, gt0, n_kept_out, flags_out, out);
}

// the second launch of such a part: fix_mask holds W words of haplotype ids per fix
int vgmi_hmm_part_fix_rows_ploidy_wide(vgmi_hmm_part* part, uint64_t n, const uint64_t* rows, const uint32_t* fix_off, const uint32_t* fix_j, const uint64_t* fix_mask)
{
    if (!part || (n && (!rows || !fix_off))) return VGMI_E_INVALID;
    if (!part->per_window_lists || !part->wide_words) return fail(part->c, VGMI_E_STATE, "HMM emissions: this part is none of vgmi_hmm_emissions_select_ploidy_wide");
    if (n == 0) return VGMI_OK;
    return hmm_fix_rows(part, n, rows, fix_off, fix_j, fix_mask, part->wide_words);
}

int vgmi_hmm_tallies_ploidy_wide(vgmi_ctx* c, uint32_t bit_len, uint32_t ploidy, uint32_t n_gt, uint32_t n_windows, const uint32_t* win_n_gt, const uint8_t* win_haps,
                                 const uint64_t* win_sel_mask, uint64_t n_rows, const uint64_t* entry_begin, const uint32_t* entry_count, const uint32_t* row_win,
                                 const uint32_t* winner, int use_alive, uint32_t* out, uint8_t* unique_out)
{
    return hmm_tallies_ploidy_impl(c, HmmForm{true, bit_len}, ploidy, n_gt, n_windows, win_n_gt, win_haps, win_sel_mask, n_rows, entry_begin, entry_count, row_win,
                                   winner, use_alive, out, unique_out);
}

int vgmi_hmm_part_fetch(vgmi_hmm_part* part, void* obs_out)
{
    if (!part || !obs_out) return VGMI_E_INVALID;
    vgmi_ctx* c = part->c;
    HIPCHK(c, hipSetDevice(c->device));
    if (part->n_rows) HIPCHK(c, hipMemcpy(obs_out, part->d_obs, (size_t)part->n_rows * part->n_gt * 16, hipMemcpyDeviceToHost));
    return VGMI_OK;
}

void vgmi_hmm_part_free(vgmi_hmm_part* part)
{
    if (!part) return;
    hmm_block_give(part->c, part->d_obs, part->obs_bytes);      // kept for the next part / sample (hipFree would wait for every stream)
    hmm_block_give(part->c, part->d_small, part->small_bytes);
    delete part;
}

int vgmi_hmm_recursion(vgmi_ctx* c, uint32_t n_gt, uint32_t ploidy, const uint8_t* keep, uint32_t n_windows, const void* obs,
                       uint64_t n_rows, const uint32_t* row, const uint8_t* restart, const void* pow, uint64_t n_steps,
                       const void* uniform, const vgmi_hmm_chain* chains, uint32_t n_chains, void* out)
{
    if (!out) return VGMI_E_INVALID;
    return hmm_run(c, n_gt, ploidy, keep, n_windows, obs, 0, n_rows, row, restart, pow, 0, n_steps, uniform, chains, n_chains, out, nullptr,
                   nullptr, nullptr, nullptr, nullptr, nullptr);
}

// ---- the recursion under `-m fre` (src/genotype.cpp:1196-1215, 1297-1316): r_g = sum over p of ((prev_p * obs_g) * f_g0) * f_g1 ..., the
// factors of genotype g from table chains[i].keep_index: freq[(t * n_gt + g) * ploidy + q], long doubles (the sampler's doubles, widened)
int vgmi_hmm_recursion_fre(vgmi_ctx* c, uint32_t n_gt, uint32_t ploidy, const void* freq, uint32_t n_tables, const void* obs, uint64_t n_rows,
                           const uint32_t* row, const uint8_t* restart, uint64_t n_steps, const void* uniform, const vgmi_hmm_chain* chains,
                           uint32_t n_chains, void* out)
{
    if (!out) return VGMI_E_INVALID;
    return hmm_run(c, n_gt, ploidy, nullptr, n_tables, obs, 0, n_rows, row, restart, nullptr, 0, n_steps, uniform, chains, n_chains, out, nullptr, nullptr,
                   nullptr, nullptr, nullptr, nullptr, nullptr, freq, true);
}

int vgmi_hmm_calls(vgmi_ctx* c, uint32_t n_gt, uint32_t ploidy, const uint8_t* keep, uint32_t n_windows, const void* obs, uint64_t n_rows,
                   const uint32_t* row, const uint8_t* restart, const void* pow, uint64_t n_steps, const void* uniform,
                   const vgmi_hmm_chain* chains, uint32_t n_chains, const uint8_t* gid, const uint8_t* order, const uint64_t* fwd_step,
                   const uint64_t* bwd_step, void* prob, uint32_t* winner, void* alpha_beta_or_null)
{
    if (!gid || !order || !fwd_step || !bwd_step || !prob || !winner) return VGMI_E_INVALID;
    return hmm_run(c, n_gt, ploidy, keep, n_windows, obs, 0, n_rows, row, restart, pow, 0, n_steps, uniform, chains, n_chains, alpha_beta_or_null,
                   gid, order, fwd_step, bwd_step, prob, winner);
}

int vgmi_hmm_calls_part(vgmi_ctx* c, uint32_t n_gt, uint32_t ploidy, const uint8_t* keep, uint32_t n_windows, const void* obs, uint64_t row_lo,
                        uint64_t row_hi, const uint32_t* row, const uint8_t* restart, const void* pow, uint64_t step_lo, uint64_t step_hi,
                        const void* uniform, const vgmi_hmm_chain* chains, uint32_t n_chains, const uint8_t* gid, const uint8_t* order,
                        const uint64_t* fwd_step, const uint64_t* bwd_step, void* prob, uint32_t* winner)
{
    if (!gid || !order || !fwd_step || !bwd_step || !prob || !winner) return VGMI_E_INVALID;
    return hmm_run(c, n_gt, ploidy, keep, n_windows, obs, row_lo, row_hi, row, restart, pow, step_lo, step_hi, uniform, chains, n_chains, nullptr,
                   gid, order, fwd_step, bwd_step, prob, winner);
}

}  // extern "C"
