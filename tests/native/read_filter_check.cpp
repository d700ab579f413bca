// Stand-alone check of csrc/vgmi_read_filter.h (built with -fsanitize=address,undefined by tests/test_read_filter_cpu.py; not loaded
// into Python).  What it prints is compared with the Python model of tests/read_filter_cases.py:
//   read_filter_check table                 the 931 entries of E10, one per line
//   read_filter_check tenths TEXT...        per TEXT: its value in tenths, or "refused"
//   read_filter_check classify FILE         FILE: first line "min_len max_len min_mean_q lowq_below lowq_max_pct", then a record per
//                                           line: "F HEX" (FASTQ quality bytes), "B HEX" (BAM QUAL bytes) or "N LEN" (no qualities);
//                                           per record "class n_low sum_e"
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "vgmi_read_filter.h"

static int hexval(char c) { return c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : -1; }

int main(int argc, char** argv)
{
    if (argc >= 2 && !strcmp(argv[1], "table")) {
        for (uint32_t t = 0; t <= VGH_READ_FILTER_MAX_TENTHS; ++t) printf("%" PRIu32 "\n", vgh::read_filter_e10(t));
        // a base's weight is the table's every tenth entry, and the clamps are where the rule says
        for (uint32_t q = 0; q <= 93; ++q)
            if (vgh::read_filter_e(q) != vgh::read_filter_e10(10 * q)) return 2;
        if (vgh::read_filter_q_fastq(0) != 0 || vgh::read_filter_q_fastq(32) != 0 || vgh::read_filter_q_fastq(33) != 0 || vgh::read_filter_q_fastq(126) != 93 ||
            vgh::read_filter_q_fastq(127) != 93 || vgh::read_filter_q_fastq(255) != 93 || vgh::read_filter_q_bam(93) != 93 || vgh::read_filter_q_bam(94) != 93 ||
            vgh::read_filter_q_bam(254) != 93 || vgh::read_filter_q_bam(0) != 0)
            return 3;
        return 0;
    }
    if (argc >= 2 && !strcmp(argv[1], "tenths")) {
        for (int i = 2; i < argc; ++i) {
            uint32_t t = 0;
            if (vgh::read_filter_parse_tenths(argv[i], &t)) printf("%" PRIu32 "\n", t);
            else printf("refused\n");
        }
        return 0;
    }
    if (argc != 3 || strcmp(argv[1], "classify")) {
        fprintf(stderr, "usage: read_filter_check table | tenths TEXT... | classify FILE\n");
        return 1;
    }
    std::ifstream in(argv[2]);
    std::string line;
    if (!std::getline(in, line)) return 1;
    uint32_t v[5] = {0, 0, 0, 0, 0};
    {
        std::istringstream ss(line);
        for (auto& x : v) ss >> x;
    }
    if (const int bad = vgh::read_filter_invalid(v[0], v[1], v[2], v[3], v[4])) {
        printf("invalid %d %s\n", bad, vgh::read_filter_invalid_text(bad));
        return 0;
    }
    const vgh::ReadFilterParams p = vgh::read_filter_params(v[0], v[1], v[2], v[3], v[4]);
    vgh::ReadFilterRule rule(p);
    while (std::getline(in, line)) {
        if (line.size() < 2) continue;
        const char kind = line[0];
        uint64_t n_low = 0, sum_e = 0;
        int cls;
        if (kind == 'N') {
            cls = vgh::read_filter_class(p, nullptr, strtoull(line.c_str() + 2, nullptr, 10), false, &n_low, &sum_e);
        } else {
            std::vector<unsigned char> q((line.size() - 2) / 2);      // (exactly the record's bytes: a read past them is the sanitizer's to find)
            for (size_t i = 0; i < q.size(); ++i) q[i] = (unsigned char)(hexval(line[2 + 2 * i]) << 4 | hexval(line[3 + 2 * i]));
            cls = vgh::read_filter_class(p, q.data(), q.size(), kind == 'B', &n_low, &sum_e);
        }
        ++rule.n_class[cls];
        printf("%d %" PRIu64 " %" PRIu64 "\n", cls, n_low, sum_e);
    }
    printf("evaluated %" PRIu64 " kept %" PRIu64 "\n", rule.evaluated(), rule.n_class[vgh::READ_PASS]);
    return 0;
}
