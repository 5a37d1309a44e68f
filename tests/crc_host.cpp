// Host program over csrc/snapmi_crc.hpp for tests/test_crc_long_cpu.py: the
// masked CRC32C of a byte range the way snapmi_crc32c_masked_batch computes
// it on the device - segments, every segment's state from a zero register,
// advanced past its tail, XORed together in no particular order, the initial
// state's term from segment 0 - and the plan arithmetic on its own.
//
//   crc_host DATAFILE < jobs
//
// One job per line, one line of answer each:
//   const                      -> kCrcSegment kCrcShort
//   crc OFF LEN SEG            -> masked CRC (8 hex digits) of data[OFF, OFF+LEN)
//   count SEG LEN              -> segments, bytes of the first one (0 0: none)
//   find SEG S LEN0 LEN1 ...   -> buffer segment off len tail of the call's
//                                 segment S
//   first SEG LEN0 LEN1 ...    -> the scan first[0..n]
//   pow T                      -> x^(8 T) mod P (8 hex digits)
//   mul A B                    -> A * B mod P (8 hex digits)
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../rust-snappy_amd/csrc/snapmi_crc.hpp"

using namespace snapmi;

static uint32_t byte_tab[256];
static uint32_t pow2[64];

// the CRC register over d[0, n), from a zero register
static uint32_t zero_state(const uint8_t *d, uint64_t n)
{
    uint32_t s = 0;
    for (uint64_t i = 0; i < n; i++)
        s = byte_tab[(s ^ d[i]) & 255] ^ (s >> 8);
    return s;
}

static std::vector<uint64_t> scan(const std::vector<uint64_t> &lens,
                                  uint64_t seg)
{
    std::vector<uint64_t> first(lens.size() + 1, 0);
    for (size_t i = 0; i < lens.size(); i++)
        first[i + 1] = first[i] + crc_segments(lens[i], seg);
    return first;
}

static uint32_t masked(const uint8_t *d, uint64_t len, uint64_t seg)
{
    const std::vector<uint64_t> lens = {len};
    const std::vector<uint64_t> first = scan(lens, seg);
    if (first[1] == 0) // the one-wavefront route
        return crc_mask(zero_state(d, len) ^
                        crc_init_term(crc_pow8(pow2, len)));
    uint32_t acc = 0;
    // (odd segments first, then the even ones from the back: XOR has no order)
    for (int pass = 1; pass >= 0; pass--)
        for (uint64_t k = first[1]; k-- > 0;) {
            if ((k & 1) != (uint64_t)pass)
                continue;
            const CrcSeg g =
                crc_find_segment(first.data(), lens.data(), 1, k, seg);
            uint32_t v = crc_advance(zero_state(d + g.off, g.len),
                                     crc_pow8(pow2, g.tail));
            if (g.segment == 0)
                v ^= crc_init_term(crc_pow8(pow2, len));
            acc ^= v;
        }
    return crc_mask(acc);
}

int main(int argc, char **argv)
{
    if (argc != 2) {
        fprintf(stderr, "usage: crc_host DATAFILE < jobs\n");
        return 2;
    }
    for (uint32_t i = 0; i < 256; i++) {
        uint32_t c = i;
        for (int k = 0; k < 8; k++)
            c = (c & 1) ? (c >> 1) ^ kCrcPoly : c >> 1;
        byte_tab[i] = c;
    }
    crc_pow2_table(pow2);
    std::vector<uint8_t> data;
    if (FILE *f = fopen(argv[1], "rb")) {
        uint8_t buf[65536];
        size_t k;
        while ((k = fread(buf, 1, sizeof buf, f)) > 0)
            data.insert(data.end(), buf, buf + k);
        fclose(f);
    } else {
        perror(argv[1]);
        return 2;
    }
    char line[1 << 16];
    while (fgets(line, sizeof line, stdin)) {
        std::vector<uint64_t> v;
        char *tok = strtok(line, " \n");
        if (!tok)
            continue;
        const std::string job = tok;
        while ((tok = strtok(nullptr, " \n")))
            v.push_back(strtoull(tok, nullptr, 10));
        if (job == "const") {
            printf("%llu %llu\n", (unsigned long long)kCrcSegment,
                   (unsigned long long)kCrcShort);
        } else if (job == "crc" && v.size() == 3 && v[0] <= data.size() &&
                   v[1] <= data.size() - v[0] && v[2]) {
            printf("%08x\n", masked(data.data() + v[0], v[1], v[2]));
        } else if (job == "count" && v.size() == 2 && v[0]) {
            const uint64_t k = crc_segments(v[1], v[0]);
            printf("%llu %llu\n", (unsigned long long)k,
                   (unsigned long long)(k ? crc_first_len(v[1], v[0]) : 0));
        } else if (job == "find" && v.size() >= 3 && v[0]) {
            const std::vector<uint64_t> lens(v.begin() + 2, v.end());
            const std::vector<uint64_t> first = scan(lens, v[0]);
            if (v[1] >= first.back()) {
                printf("none\n");
                continue;
            }
            const CrcSeg g = crc_find_segment(first.data(), lens.data(),
                                              (uint32_t)lens.size(), v[1],
                                              v[0]);
            printf("%u %llu %llu %llu %llu\n", g.buffer,
                   (unsigned long long)g.segment, (unsigned long long)g.off,
                   (unsigned long long)g.len, (unsigned long long)g.tail);
        } else if (job == "first" && v.size() >= 1 && v[0]) {
            const std::vector<uint64_t> lens(v.begin() + 1, v.end());
            for (uint64_t x : scan(lens, v[0]))
                printf("%llu ", (unsigned long long)x);
            printf("\n");
        } else if (job == "pow" && v.size() == 1) {
            printf("%08x\n", crc_pow8(pow2, v[0]));
        } else if (job == "mul" && v.size() == 2) {
            printf("%08x\n", gf_mul((uint32_t)v[0], (uint32_t)v[1]));
        } else {
            printf("bad job\n");
        }
    }
    return 0;
}
