// Host build of csrc/snapmi_framewalk.hpp for
// tests/test_frame_host_batch_cpu.py: the chunk-header walk the kernels of
// snapmi_framedec.hip run, driven the way snapmi_hostbatch.hip drives it while it
// stages a framed stream.
#include <stdint.h>
#include <stddef.h>

#include "../rust-snappy_amd/csrc/snapmi_framewalk.hpp"

using namespace snapmi;

extern "C" {

uint64_t t_entry_bytes(void) { return sizeof(FwEntry); }

// frame_walk_host of one stream.  out: kind, a, b of the walk's verdict, the
// room, the data chunks in front of the verdict; entries: (header offset,
// header word) of the first `cap` of them.
void t_walk(const uint8_t *in, uint64_t len, uint64_t *out, uint64_t *entries,
            uint64_t cap)
{
    uint64_t k = 0;
    const FwStream w =
        frame_walk_host(in, len, [&](uint64_t off, uint32_t hd) {
            if (k < cap) {
                entries[2 * k] = off;
                entries[2 * k + 1] = hd;
            }
            k++;
        });
    out[0] = (uint64_t)(int64_t)w.e.kind;
    out[1] = w.e.a;
    out[2] = w.e.b;
    out[3] = w.room;
    out[4] = w.chunks;
    out[5] = k;
}

// frame_index_walk: what snapmi_frame_index_host answers
int t_index(const uint8_t *in, uint64_t len, uint64_t *offsets, uint64_t cap,
            uint64_t *n_chunks)
{
    return frame_index_walk(in, len, offsets, cap, n_chunks);
}

} // extern "C"
