// Stand-alone host build of the range-write rules (bi_write_*) of
// csrc/snapmi_blockindex.hpp for tests/test_write_index_cpu.py: one command
// per line of standard input, one line of answer each, as the kernels and the
// host entry point call them.  A write list is "m" followed by m triples
// "stream off len".
//   C n m writes...        -> code bad         (bi_write_check; bad 0 when OK)
//   N m writes...          -> the touched blocks, saturating (any list)
//   T m writes...          -> count, then "stream block write edge" for every
//                             touched block of a CHECKED list
//   S off len k            -> edge from to n   (k a touched block of the write)
//   K in_len blocks e...   -> first bad block, or 18446744073709551615
//   X hdr_old hdr_new blocks nt e[blocks + 1] tk[nt] tsize[nt]
//                          -> the new entries by bi_write_splice, then the
//                             same by bi_write_entry (2 * (blocks + 1) numbers)
//   F cap new_len          -> 0 / 1
//   G scratch m writes...  -> bi_update_groups of a CHECKED list, as the entry
//                             point calls it: the count, "t0 tg b0 bg rooms"
//                             for every group, the three maxima, then the
//                             room of every touched block (4294967295: covered)
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

struct Writes {
    std::vector<uint32_t> stream;
    std::vector<uint64_t> off, len;
};

// the list behind a[at]: m, then m triples - exactly to the end of the line
static bool writes_at(const std::vector<uint64_t> &a, size_t at, Writes *w)
{
    if (a.size() <= at || a.size() != at + 1 + 3 * a[at])
        return false;
    for (uint64_t i = 0; i < a[at]; i++) {
        w->stream.push_back((uint32_t)a[at + 1 + 3 * i]);
        w->off.push_back(a[at + 2 + 3 * i]);
        w->len.push_back(a[at + 3 + 3 * i]);
    }
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
        Writes w;
        if (op == 'C' && writes_at(a, 1, &w)) {
            size_t bad = 0;
            const int code =
                bi_write_check(w.stream.data(), w.off.data(), w.len.data(),
                               w.off.size(), a[0], &bad);
            printf("%d %zu\n", code, code ? bad : (size_t)0);
        } else if (op == 'N' && writes_at(a, 0, &w)) {
            BiWriteWalk walk;
            uint64_t sum = 0;
            for (size_t i = 0; i < w.off.size(); i++) {
                if (w.len[i] == 0)
                    continue;
                uint64_t k0;
                const uint64_t c = bi_write_touch(walk, w.stream[i], w.off[i],
                                                  w.len[i], &k0);
                sum = sum + c < sum ? ~0ull : sum + c;
            }
            printf("%" PRIu64 "\n", sum);
        } else if (op == 'T' && writes_at(a, 0, &w)) {
            BiWriteWalk walk;
            std::vector<uint64_t> out;
            for (size_t i = 0; i < w.off.size(); i++) {
                if (w.len[i] == 0)
                    continue;
                uint64_t k0;
                const uint64_t c = bi_write_touch(walk, w.stream[i], w.off[i],
                                                  w.len[i], &k0);
                for (uint64_t k = k0; k < k0 + c; k++) {
                    out.push_back(w.stream[i]);
                    out.push_back(k);
                    out.push_back(i);
                    out.push_back(bi_write_edge(w.off[i], w.len[i], k));
                }
            }
            printf("%zu", out.size() / 4);
            for (uint64_t x : out)
                printf(" %" PRIu64, x);
            printf("\n");
        } else if (op == 'S' && a.size() == 3) {
            const BiSpan s = bi_write_span(a[0], a[1], a[2]);
            printf("%d %" PRIu64 " %" PRIu64 " %" PRIu64 "\n",
                   bi_write_edge(a[0], a[1], a[2]) ? 1 : 0, s.from, s.to, s.n);
        } else if (op == 'K' && a.size() >= 2 && a.size() == 2 + a[1] + 1) {
            printf("%" PRIu64 "\n",
                   bi_write_first_bad_block(a.data() + 2, a[0], a[1]));
        } else if (op == 'X' && a.size() >= 4 &&
                   a.size() == 4 + a[2] + 1 + 2 * a[3]) {
            const uint32_t hdr_old = (uint32_t)a[0], hdr_new = (uint32_t)a[1];
            const uint64_t blocks = a[2], nt = a[3];
            const uint64_t *e = a.data() + 4, *tk = e + blocks + 1,
                           *tsize = tk + nt;
            std::vector<uint64_t> e_new(blocks + 1), tcum(nt + 1);
            const uint64_t end =
                bi_write_splice(e, blocks, tk, tsize, nt, hdr_new,
                                e_new.data());
            if (end != e_new[blocks])
                return 3;
            // (what k_write_sizes sums: new size - old size, modulo 2^64)
            tcum[0] = 0;
            for (uint64_t j = 0; j < nt; j++)
                tcum[j + 1] =
                    tcum[j] + tsize[j] - (e[tk[j] + 1] - e[tk[j]]);
            for (uint64_t k = 0; k <= blocks; k++)
                printf("%" PRIu64 " ", e_new[k]);
            for (uint64_t k = 0; k <= blocks; k++)
                printf("%" PRIu64 "%c",
                       bi_write_entry(e, k, tk, tcum.data(), nt, hdr_old,
                                      hdr_new),
                       k == blocks ? '\n' : ' ');
        } else if (op == 'F' && a.size() == 2) {
            printf("%d\n", bi_write_fits(a[0], a[1]) ? 1 : 0);
        } else if (op == 'G' && writes_at(a, 1, &w)) {
            // the touched streams: the first block and the rooms of each
            BiWriteWalk walk;
            std::vector<uint32_t> ts_stream, ts_b0, ts_rooms;
            std::vector<uint8_t> edge;
            for (size_t i = 0; i < w.off.size(); i++) {
                if (w.len[i] == 0)
                    continue;
                if (ts_stream.empty() || ts_stream.back() != w.stream[i]) {
                    ts_stream.push_back(w.stream[i]);
                    ts_b0.push_back((uint32_t)edge.size());
                    ts_rooms.push_back(0);
                }
                uint64_t k0;
                const uint64_t c = bi_write_touch(walk, w.stream[i], w.off[i],
                                                  w.len[i], &k0);
                for (uint64_t k = k0; k < k0 + c; k++) {
                    edge.push_back(bi_write_edge(w.off[i], w.len[i], k));
                    ts_rooms.back() += edge.back();
                }
            }
            ts_b0.push_back((uint32_t)edge.size());
            const size_t ts = ts_stream.size();
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
            for (size_t t = 0; t < ts; t++) {
                uint32_t r = room0[t];
                for (uint32_t b = ts_b0[t]; b < ts_b0[t + 1]; b++)
                    printf(" %u", edge[b] ? r++ : 0xFFFFFFFFu);
            }
            printf("\n");
        } else {
            return 2;
        }
    }
    return 0;
}
