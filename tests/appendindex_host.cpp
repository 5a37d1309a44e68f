// Stand-alone host build of the append rules (bi_append_*) of
// csrc/snapmi_blockindex.hpp for tests/test_append_index_cpu.py: one command
// per line of standard input, one line of answer each, as the kernels and the
// host entry point call them.
//   L dlen add             -> entries kf tail fill blocks
//   B dlen add j           -> room off len in_len   (j a new block)
//   C index_entries n (dlen add) * n
//                          -> code bad entries blocks   (bi_append_check; bad,
//                             entries, blocks 0 where the code leaves them)
//   K in_len blocks e...   -> first bad block, or 18446744073709551615
//   X hdr_old hdr_new kf nb e[kf + 1] nsize[nb]
//                          -> the new entries by bi_append_splice, then the
//                             same by bi_append_entry (2 * (kf + nb + 1)
//                             numbers)
//   F cap new_len          -> 0 / 1
//   G scratch n (dlen add) * n
//                          -> bi_update_groups as the entry point calls it:
//                             the count, "t0 tg b0 bg rooms" for every group,
//                             the three maxima, then the room of every named
//                             stream (4294967295: no tail)
// (it has a main of its own so that it can also be built with
// -fsanitize=address,undefined and run as it is)
#include <inttypes.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

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
        if (op == 'L' && a.size() == 2) {
            printf("%" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64
                   "\n",
                   bi_append_entries(a[0], a[1]), bi_append_full(a[0]),
                   bi_append_tail(a[0]), bi_append_fill(a[0], a[1]),
                   bi_append_blocks(a[0], a[1]));
        } else if (op == 'B' && a.size() == 3) {
            const BiAppendBlock b = bi_append_block(a[0], a[1], a[2]);
            printf("%d %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", b.room ? 1 : 0,
                   b.off, b.len, b.in_len);
        } else if (op == 'C' && a.size() >= 2 && a.size() == 2 + 2 * a[1]) {
            const size_t n = (size_t)a[1];
            std::vector<uint64_t> out(n), add(n);
            for (size_t i = 0; i < n; i++) {
                out[i] = a[2 + 2 * i];
                add[i] = a[3 + 2 * i];
            }
            size_t bad = 0;
            uint64_t entries = 0, blocks = 0;
            const int code = bi_append_check(out.data(), add.data(), n, a[0],
                                             &entries, &blocks, &bad);
            printf("%d %zu %" PRIu64 " %" PRIu64 "\n", code, bad, entries,
                   blocks);
        } else if (op == 'K' && a.size() >= 2 && a.size() == 2 + a[1] + 1) {
            printf("%" PRIu64 "\n",
                   bi_append_first_bad_block(a.data() + 2, a[0], a[1]));
        } else if (op == 'X' && a.size() >= 4 &&
                   a.size() == 4 + a[2] + 1 + a[3]) {
            const uint32_t hdr_old = (uint32_t)a[0], hdr_new = (uint32_t)a[1];
            const uint64_t kf = a[2], nb = a[3];
            const uint64_t *e = a.data() + 4, *nsize = e + kf + 1;
            std::vector<uint64_t> e_new(kf + nb + 1), ncum(nb + 1);
            const uint64_t end =
                bi_append_splice(e, kf, nsize, nb, hdr_new, e_new.data());
            if (end != e_new[kf + nb])
                return 3;
            // (what k_append_sizes sums)
            ncum[0] = 0;
            for (uint64_t j = 0; j < nb; j++)
                ncum[j + 1] = ncum[j] + nsize[j];
            for (uint64_t k = 0; k <= kf + nb; k++)
                printf("%" PRIu64 " ", e_new[k]);
            for (uint64_t k = 0; k <= kf + nb; k++)
                printf("%" PRIu64 "%c",
                       bi_append_entry(e, k, kf, ncum.data(), hdr_old,
                                       hdr_new),
                       k == kf + nb ? '\n' : ' ');
        } else if (op == 'F' && a.size() == 2) {
            printf("%d\n", bi_append_fits(a[0], a[1]) ? 1 : 0);
        } else if (op == 'G' && a.size() >= 2 && a.size() == 2 + 2 * a[1]) {
            // the named streams: the first new block and the rooms of each
            std::vector<uint32_t> ts_b0, ts_rooms;
            uint32_t b = 0;
            for (size_t i = 0; i < (size_t)a[1]; i++) {
                const uint64_t dlen = a[2 + 2 * i], add = a[3 + 2 * i];
                if (add == 0)
                    continue;
                ts_b0.push_back(b);
                ts_rooms.push_back(bi_append_tail(dlen) ? 1 : 0);
                b += (uint32_t)bi_append_blocks(dlen, add);
            }
            ts_b0.push_back(b);
            const size_t ts = ts_rooms.size();
            std::vector<BiUpdateGroup> groups(ts);
            std::vector<uint32_t> room0(ts);
            BiUpdateMax max;
            const size_t count =
                bi_update_groups(ts_b0.data(), ts_rooms.data(), ts, a[0],
                                 groups.data(), room0.data(), &max);
            printf("%zu", count);
            for (size_t q = 0; q < count; q++)
                printf(" %u %u %u %u %u", groups[q].t0, groups[q].tg,
                       groups[q].b0, groups[q].bg, groups[q].rooms);
            printf(" %" PRIu64 " %" PRIu64 " %" PRIu64, max.tg, max.bg,
                   max.rooms);
            for (size_t t = 0; t < ts; t++)
                printf(" %u", ts_rooms[t] ? room0[t] : 0xFFFFFFFFu);
            printf("\n");
        } else {
            return 2;
        }
    }
    return 0;
}
