// Stand-alone host build of csrc/snapmi_element.hpp for
// tests/test_element_cpu.py: lane_decode (what the lane kernels run on global
// memory) over plain host memory, and the walker.
//
// argv[1]: a file of cases, little endian: u32 count, then per case
//   u64 cap, u32 len, len bytes (a raw stream).
// Answer per case, one line each:
//   flat <kind> <a> <b> <c> <out_len> <crc32 of the output>
//   piece ...   the same for the elements behind the header as a headerless
//       piece (mode 2) that must produce exactly the announced length - how
//       the kernels mostly run this loop; "piece -" without a header
//   walk <ok> <p> <out> <elements>   elem_step from behind the header until
//       the stream's end or the first element that does not fit ("walk -"
//       without a header)
// and, with argv[1] = "tags": per tag byte "<tag> <encoded> <produced>".
// Every buffer is an allocation of exactly its size, so that the sanitizer
// build sees any byte read or written outside of it.
#include <inttypes.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../rust-snappy_amd/csrc/snapmi_element.hpp"

using namespace snapmi;

static uint32_t crc32(const uint8_t *p, size_t n)
{
    uint32_t c = 0xFFFFFFFFu;
    for (size_t i = 0; i < n; i++) {
        c ^= p[i];
        for (int k = 0; k < 8; k++)
            c = (c >> 1) ^ (0xEDB88320u & (0u - (c & 1)));
    }
    return ~c;
}

static void answer(const char *who, const snapmi_error &e, const uint8_t *out,
                   uint64_t out_len)
{
    printf("%s %d %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %u\n", who,
           e.kind, e.a, e.b, e.c, out_len, crc32(out, (size_t)out_len));
}

// an allocation of exactly n bytes (never a null pointer)
struct Exact {
    uint8_t *p;
    explicit Exact(size_t n) : p((uint8_t *)malloc(n ? n : 1))
    {
        if (!p)
            abort();
    }
    ~Exact() { free(p); }
};

static void flat(const uint8_t *in, uint64_t in_len, uint64_t cap)
{
    Exact dst((size_t)cap);
    snapmi_error e;
    memset(&e, 0, sizeof e);
    uint64_t produced = 0;
    const bool ok = lane_decode(in, in_len, 0, dst.p, cap, &produced, &e, 0);
    if (ok != (e.kind == SNAPMI_OK) || (!ok && produced != 0))
        abort();
    answer("flat", e, dst.p, produced);
}

static void piece(const uint8_t *in, uint64_t in_len, uint64_t cap)
{
    snapmi_error e;
    memset(&e, 0, sizeof e);
    uint32_t hdr = 0;
    uint64_t dl = 0, produced = 0;
    if (header_read(bytes_at(in), in_len, &hdr, &dl, &e, 0) != SNAPMI_OK ||
        dl > cap) {
        printf("piece -\n");
        return;
    }
    Exact dst((size_t)dl);
    lane_decode(in + hdr, in_len - hdr, 2, dst.p, dl, &produced, &e, 0);
    answer("piece", e, dst.p, produced);
}

static void walk(const uint8_t *in, uint64_t in_len)
{
    uint64_t dl = 0;
    const uint32_t hdr = varint_read(bytes_at(in), in_len, &dl);
    if (hdr == 0) {
        printf("walk -\n");
        return;
    }
    uint64_t p = hdr, out = 0, n = 0;
    bool ok = true;
    while (ok && p < in_len) {
        ok = elem_step(bytes_at(in), in_len, p, out);
        n += ok;
    }
    printf("walk %d %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", ok ? 1 : 0, p, out,
           n);
}

int main(int argc, char **argv)
{
    if (argc != 2)
        return 2;
    if (!strcmp(argv[1], "tags")) {
        for (uint32_t t = 0; t < 256; t++)
            printf("%u %u %u\n", t, tag_encoded(t), tag_produced(t));
        return 0;
    }
    FILE *f = fopen(argv[1], "rb");
    if (!f)
        return 2;
    uint32_t count = 0;
    if (fread(&count, 4, 1, f) != 1)
        abort();
    for (uint32_t i = 0; i < count; i++) {
        uint64_t cap = 0;
        uint32_t len = 0;
        if (fread(&cap, 8, 1, f) != 1 || fread(&len, 4, 1, f) != 1)
            abort();
        Exact in(len);
        if (len && fread(in.p, 1, len, f) != len)
            abort();
        flat(in.p, len, cap);
        piece(in.p, len, cap);
        walk(in.p, len);
    }
    fclose(f);
    return 0;
}
