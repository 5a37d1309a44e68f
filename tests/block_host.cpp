// Stand-alone host build of csrc/snapmi_block.hpp for tests/test_block_cpu.py:
// CompressArgs over plain host arrays, the block rules asked for every block.
//
// Standard input, one case after the other:
//   batch <n> <direct> <host_blocks> <host_slots> <blk_lo> <blk_hi>
//   <n lengths> <n + 1 blk_first> <n + 1 slot_first> <blk_first[n] + 1 blk_off>
// answers
//   launch <launch_blocks> <segment_blocks>
//   one line per block b < blk_first[n], as the plan on the device counted:
//     <b> <st> <k> <total> <n> <off> <where>
//   with <where> = "out <stream> <offset>" (the caller's output of that
//   stream, found by address), "slot <offset>" (scratch), "none" (block_dest
//   said no) or "past" (b >= launch_blocks: no kernel asks for it), then
//   one line per stream: head <the first 10 bytes of its output, hex>
//   (0xEE where nothing was written: only varint(total) ever is).
//   table <n> <cap>
// answers
//   <shift> <size>
// The test's model is not known here: where a pointer lies is found from the
// buffers alone.
#include <inttypes.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../rust-snappy_amd/csrc/snapmi_block.hpp"

using namespace snapmi;

template <class T> static std::vector<T> numbers(size_t count)
{
    std::vector<T> v(count);
    for (size_t i = 0; i < count; i++) {
        unsigned long long x;
        if (scanf("%llu", &x) != 1)
            abort();
        v[i] = (T)x;
    }
    return v;
}

static void batch()
{
    unsigned long long n, direct, host_blocks, host_slots, blk_lo, blk_hi;
    if (scanf("%llu %llu %llu %llu %llu %llu", &n, &direct, &host_blocks,
              &host_slots, &blk_lo, &blk_hi) != 6)
        abort();
    std::vector<uint64_t> lens = numbers<uint64_t>(n);
    std::vector<uint32_t> blk_first = numbers<uint32_t>(n + 1);
    std::vector<uint32_t> slot_first = numbers<uint32_t>(n + 1);
    std::vector<uint64_t> blk_off = numbers<uint64_t>(blk_first[n] + 1);

    // every stream's output with room for the worst case, apart from each
    // other; the scratch slots the host sized
    std::vector<std::vector<uint8_t>> outs(n);
    std::vector<void *> out_ptrs(n);
    std::vector<const void *> in_ptrs(n);
    std::vector<std::vector<uint8_t>> ins(n);
    for (size_t i = 0; i < n; i++) {
        outs[i].assign((size_t)max_compress_len_u64(lens[i]) + 16, 0xEE);
        out_ptrs[i] = outs[i].data();
        ins[i].assign((size_t)lens[i] + 1, 0);
        in_ptrs[i] = ins[i].data();
    }
    std::vector<uint8_t> scratch((size_t)host_slots * kSlotBytes + 16, 0xEE);

    CompressArgs a;
    memset(&a, 0, sizeof a);
    a.in_ptrs = in_ptrs.data();
    a.in_lens = lens.data();
    a.out_ptrs = out_ptrs.data();
    a.blk_first = blk_first.data();
    a.slot_first = slot_first.data();
    a.blk_off = blk_off.data();
    a.scratch = scratch.data();
    a.n_streams = (uint32_t)n;
    a.host_blocks = (uint32_t)host_blocks;
    a.host_slots = (uint32_t)host_slots;
    a.blk_lo = (uint32_t)blk_lo;
    a.blk_hi = (uint32_t)blk_hi;
    a.direct = (uint32_t)direct;

    printf("launch %u %u\n", launch_blocks(a), segment_blocks(a));
    for (uint32_t b = 0; b < blk_first[n]; b++) {
        const BlockAt at = locate_block(a, b);
        printf("%u %u %u %" PRIu64 " %u %" PRIu64 " ", b, at.st, at.k,
               at.total, at.n,
               (uint64_t)((const uint8_t *)at.in + at.off() -
                          ins[at.st].data()));
        uint8_t *dst = nullptr;
        if (b >= launch_blocks(a)) {
            printf("past\n");
        } else if (!block_dest(a, at, b, true, dst)) {
            printf("none\n");
        } else if (dst >= scratch.data() &&
                   dst < scratch.data() + scratch.size()) {
            printf("slot %zu\n", (size_t)(dst - scratch.data()));
        } else {
            size_t i = 0;
            while (i < n && !(dst >= outs[i].data() &&
                              dst < outs[i].data() + outs[i].size()))
                i++;
            if (i == n)
                abort(); // a destination in nobody's memory
            printf("out %zu %zu\n", i, (size_t)(dst - outs[i].data()));
        }
    }
    for (size_t i = 0; i < n; i++) {
        printf("head ");
        for (size_t j = 0; j < 10; j++)
            printf("%02x", outs[i][j]);
        printf("\n");
        for (size_t j = 10; j < outs[i].size(); j++)
            if (outs[i][j] != 0xEE)
                abort(); // more than a varint was written
    }
    for (uint8_t x : scratch)
        if (x != 0xEE)
            abort(); // the rules write nothing into a slot
}

int main()
{
    char word[16];
    while (scanf("%15s", word) == 1) {
        if (!strcmp(word, "batch")) {
            batch();
        } else if (!strcmp(word, "table")) {
            unsigned long long n, cap;
            if (scanf("%llu %llu", &n, &cap) != 2)
                abort();
            const TableShape t = table_shift((uint32_t)n, (uint32_t)cap);
            printf("%u %u\n", t.shift, t.size);
        } else {
            abort();
        }
    }
    return 0;
}
