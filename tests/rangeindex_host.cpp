// Stand-alone host build of the range-read rules of
// csrc/snapmi_blockindex.hpp for tests/test_range_index_cpu.py: one command
// per line of standard input, one line of answer each, as the kernels and
// the host entry point call them.
//   B off len              -> count k0 edges
//   E off len k            -> edge slot from to n        (k a touched block)
//   U in_len hdr dlen first next total e...  -> 0 / 1    (e: the whole index)
//   K in_len off len e...  -> first bad block, or 18446744073709551615
//   P m off len ...        -> the pieces of m ranges, saturating
//   G scratch m off len ...  -> groups max_pieces max_rooms, then r0 mg
//                               pieces rooms of every group (bi_range_groups)
// (it has a main of its own so that it can also be built with
// -fsanitize=address,undefined and run as it is)
#include <inttypes.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <iostream>
#include <string>
#include <vector>

#include "../rust-snappy_amd/csrc/snapmi_blockindex.hpp"

using namespace snapmi;

static bool next_u64(char *&p, uint64_t *v)
{
    while (*p == ' ')
        p++;
    if (*p < '0' || *p > '9')
        return false;
    char *end = nullptr;
    *v = strtoull(p, &end, 10);
    p = end;
    return true;
}

int main()
{
    std::string line;
    while (std::getline(std::cin, line)) {
        line.push_back('\0');
        char *p = &line[0];
        const char op = *p++;
        std::vector<uint64_t> a;
        uint64_t v;
        while (next_u64(p, &v))
            a.push_back(v);
        if (op == 'B' && a.size() == 2) {
            uint64_t k0;
            const uint64_t cnt = bi_range_blocks(a[0], a[1], &k0);
            printf("%" PRIu64 " %" PRIu64 " %u\n", cnt, k0,
                   bi_range_edges(a[0], a[1]));
        } else if (op == 'E' && a.size() == 3) {
            const BiSpan s = bi_range_span(a[0], a[1], a[2]);
            printf("%d %u %" PRIu64 " %" PRIu64 " %" PRIu64 "\n",
                   bi_range_edge(a[0], a[1], a[2]) ? 1 : 0,
                   bi_range_edge_slot(a[0], a[1], a[2]), s.from, s.to, s.n);
        } else if (op == 'U' && a.size() >= 6) {
            // (the rule reads e[first] and e[next - 1] only when they lie
            // inside `total`: the vector holds exactly `total` entries)
            if (a.size() - 6 != a[5])
                return 2;
            printf("%d\n", bi_range_stream_usable(a[0], (uint32_t)a[1], a[2],
                                                  a.data() + 6, a[3], a[4],
                                                  a[5])
                               ? 1
                               : 0);
        } else if (op == 'K' && a.size() >= 3) {
            printf("%" PRIu64 "\n",
                   bi_range_first_bad_block(a.data() + 3, a[0], a[1], a[2]));
        } else if (op == 'P' && a.size() >= 1 && a.size() == 1 + 2 * a[0]) {
            std::vector<uint64_t> off(a[0]), len(a[0]);
            for (uint64_t r = 0; r < a[0]; r++) {
                off[r] = a[1 + 2 * r];
                len[r] = a[2 + 2 * r];
            }
            printf("%" PRIu64 "\n",
                   bi_range_pieces(off.data(), len.data(), off.size()));
        } else if (op == 'G' && a.size() >= 2 && a.size() == 2 + 2 * a[1]) {
            // (the arrays have exactly m places, the groups' as well)
            const size_t m = (size_t)a[1];
            std::vector<uint64_t> off(m), len(m);
            for (size_t r = 0; r < m; r++) {
                off[r] = a[2 + 2 * r];
                len[r] = a[3 + 2 * r];
            }
            std::vector<BiRangeGroup> g(m);
            BiRangeMax max;
            const size_t count = bi_range_groups(off.data(), len.data(), m,
                                                 a[0], g.data(), &max);
            if (count > m)
                return 3;
            printf("%zu %" PRIu64 " %" PRIu64, count, max.pieces, max.rooms);
            for (size_t i = 0; i < count; i++)
                printf(" %u %u %" PRIu64 " %" PRIu64, g[i].r0, g[i].mg,
                       g[i].pieces, g[i].rooms);
            printf("\n");
        } else {
            return 2;
        }
    }
    return 0;
}
