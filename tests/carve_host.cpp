// Stand-alone host build of csrc/snapmi_carve.hpp and of the layout functions
// of csrc/snapmi_frame.hpp for tests/test_carve_cpu.py.
//
// First line of the answer: sizeof(FrameChunk) sizeof(snapmi_error).
// Then the Carver alone, one line per (element size, count) of the mixed list
// 1, 4, 8, 24, 32 bytes x 0, 1, 3, 17 elements, in that order:
//   elem count bytes_before bytes_after offset address%16
// and one line "end <measured> <placed end - base>".
// Then, per line "n total seg nseg" of standard input, one line per layout:
//   <tag> <measured> <placed end - base> <base % 16> {<array> <elem> <offset>}...
// with tags streams, lone (n = 1 whatever the line says), chunks, desc0,
// desc1 (a lone stream) and crc.  Every layout is measured, then placed on a
// buffer of exactly the measured size, and the test's counts are not known
// here: the arrays are named with their element size and their offset only.
#include <inttypes.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "../rust-snappy_amd/csrc/snapmi_frame.hpp"

using namespace snapmi;

struct S24 {
    uint8_t b[24];
};
struct S32 {
    uint8_t b[32];
};

static uint8_t *g_base;

template <class T> static void put(const char *name, T *p)
{
    printf(" %s %zu %zu", name, sizeof(T), (size_t)((uint8_t *)p - g_base));
}

// a buffer of exactly `bytes` bytes (one at the least), 256-aligned
static uint8_t *buffer(size_t bytes)
{
    void *p = nullptr;
    if (posix_memalign(&p, 256, bytes ? bytes : 1))
        abort();
    return g_base = (uint8_t *)p;
}

static void head(const char *tag, const Carver &m, const Carver &p)
{
    printf("%s %zu %zu %zu", tag, m.bytes(), p.bytes(),
           (size_t)((uintptr_t)g_base % 16));
}

template <class T>
static void mixed(Carver &m, Carver &p, size_t count)
{
    const size_t before = p.bytes();
    T *x = m.take<T>(count);
    T *y = p.take<T>(count);
    if (x != nullptr)
        abort(); // a measuring pass hands out no address
    printf("%zu %zu %zu %zu %zu %zu\n", sizeof(T), count, before, p.bytes(),
           (size_t)((uint8_t *)y - g_base), (size_t)((uintptr_t)y % 16));
}

static void carver_alone()
{
    const size_t counts[4] = {0, 1, 3, 17};
    Carver m;
    Carver p(buffer(4096));
    for (size_t c : counts) {
        mixed<uint8_t>(m, p, c);
        mixed<uint32_t>(m, p, c);
        mixed<uint64_t>(m, p, c);
        mixed<S24>(m, p, c);
        mixed<S32>(m, p, c);
    }
    printf("end %zu %zu\n", m.bytes(), p.bytes());
    free(g_base);
}

static void streams(size_t n)
{
    FrameBatchDecodeArgs a;
    a.n = (uint32_t)n;
    Carver m;
    fbd_streams_layout(m, a);
    Carver p(buffer(m.bytes()));
    fbd_streams_layout(p, a);
    head("streams", m, p);
    put("counts", a.counts);
    put("first", a.first);
    put("serr", a.serr);
    put("sidx", a.sidx);
    put("first_bad", a.first_bad);
    printf("\n");
    free(g_base);
}

static void lone(size_t nseg)
{
    FrameBatchDecodeArgs b;
    FrameDecodeArgs a;
    b.n = 1;
    a.nseg = (uint32_t)nseg;
    Carver m;
    frame_lone_layout(m, b, a);
    Carver p(buffer(m.bytes()));
    frame_lone_layout(p, b, a);
    if (a.counts != b.counts || a.first != b.first || a.serr != b.serr ||
        a.sidx != b.sidx || a.first_bad != b.first_bad)
        abort(); // the lone stream's arrays are the batch of one's
    head("lone", m, p);
    put("counts", a.counts);
    put("first", a.first);
    put("serr", a.serr);
    put("sidx", a.sidx);
    put("first_bad", a.first_bad);
    put("in_ptrs", a.in_ptrs);
    put("in_lens", a.in_lens);
    put("out_ptrs", a.out_ptrs);
    put("out_caps", a.out_caps);
    put("meta", a.meta);
    put("fw_cand", a.fw_cand);
    put("fw_entry", a.fw_entry);
    put("fw_ncand", a.fw_ncand);
    put("fw_base", a.fw_base);
    printf("\n");
    free(g_base);
}

static void chunks(size_t total)
{
    FrameBatchDecodeArgs a;
    a.total = (uint32_t)total;
    Carver m;
    fbd_chunks_layout(m, a);
    Carver p(buffer(m.bytes()));
    fbd_chunks_layout(p, a);
    head("chunks", m, p);
    put("chunks", a.chunks);
    put("c_stream", a.c_stream);
    put("dlens", a.dlens);
    put("offs", a.offs);
    put("cerrs", a.cerrs);
    put("derrs", a.derrs);
    put("c_in", a.c_in);
    put("c_in_len", a.c_in_len);
    put("c_out", a.c_out);
    put("c_caps", a.c_caps);
    put("c_out_lens", a.c_out_lens);
    put("modes", a.modes);
    put("crcs", a.crcs);
    printf("\n");
    free(g_base);
}

static void desc(size_t n, size_t total, size_t seg, bool is_lone)
{
    FrameBatchCompressArgs a;
    a.in_ptrs = nullptr;
    a.in_lens = nullptr;
    a.out_ptrs = nullptr;
    a.n = (uint32_t)n;
    a.total = (uint32_t)total;
    a.seg = (uint32_t)seg;
    Carver m;
    fb_desc_layout(m, a, is_lone);
    Carver p(buffer(m.bytes()));
    const FrameLonePlaces l = fb_desc_layout(p, a, is_lone);
    if (is_lone ? (a.in_ptrs != l.in || a.in_lens != l.len ||
                   a.out_ptrs != l.out)
                : (a.in_ptrs || a.in_lens || a.out_ptrs))
        abort(); // only a lone stream's block points at the places
    head(is_lone ? "desc1" : "desc0", m, p);
    put("lone_in", l.in);
    put("lone_len", l.len);
    put("lone_out", l.out);
    put("counts", a.counts);
    put("first", a.first);
    put("refused", a.refused);
    put("sbase", a.sbase);
    put("c_in", a.c_in);
    put("c_len", a.c_len);
    put("c_stream", a.c_stream);
    put("carry", a.carry);
    put("slot_ptrs", a.slot_ptrs);
    put("clens", a.clens);
    put("crcs", a.crcs);
    put("sizes", a.sizes);
    put("offs", a.offs);
    printf("\n");
    free(g_base);
}

static void crc(size_t n)
{
    CrcLong l;
    Carver m;
    crc_long_layout(m, l, n);
    Carver p(buffer(m.bytes()));
    crc_long_layout(p, l, n);
    head("crc", m, p);
    put("seg_first", l.seg_first);
    put("acc", l.acc);
    printf("\n");
    free(g_base);
}

int main()
{
    printf("%zu %zu\n", sizeof(FrameChunk), sizeof(snapmi_error));
    carver_alone();
    unsigned long long n, total, seg, nseg;
    while (scanf("%llu %llu %llu %llu", &n, &total, &seg, &nseg) == 4) {
        streams((size_t)n);
        lone((size_t)nseg);
        chunks((size_t)total);
        desc((size_t)n, (size_t)total, (size_t)seg, false);
        desc((size_t)n, (size_t)total, (size_t)seg, true);
        crc((size_t)n);
    }
    return 0;
}
