// Host build of csrc/snapmi_hostbatch.hpp for tests/test_host_batch_cpu.py:
// the slice planner of the host-memory batch calls and the tile -> stream
// mapping of k_hb_pack, driven the way snapmi_hostbatch.hip drives them.
#include <stdint.h>
#include <stddef.h>

#include <vector>

#include "../rust-snappy_amd/csrc/snapmi_hostbatch.hpp"

using namespace snapmi;

extern "C" {

uint64_t t_tile_bytes(void) { return kHbTile; }
uint64_t t_max_slice_streams(void) { return kHbMaxSliceStreams; }

// Plans the whole batch as host_batch() does.  slices: 5 values per slice
// (s0, s1, in_raw, in_bytes, out_bytes), at most cap slices; in_offs /
// out_offs: n values, every stream's offset inside its slice's slabs.
// Returns the number of slices.
size_t t_plan(const size_t *in_lens, const uint64_t *rooms, size_t n,
              uint64_t in_limit, uint64_t out_limit, uint64_t *slices,
              size_t cap, uint64_t *in_offs, uint64_t *out_offs)
{
    size_t cursor = 0, k = 0;
    while (cursor < n) {
        const HbSlice x = hb_plan_slice(in_lens, rooms, n, cursor, in_limit,
                                        out_limit, in_offs + cursor,
                                        out_offs + cursor);
        if (k < cap) {
            slices[5 * k + 0] = x.s0;
            slices[5 * k + 1] = x.s1;
            slices[5 * k + 2] = x.in_raw;
            slices[5 * k + 3] = x.in_bytes;
            slices[5 * k + 4] = x.out_bytes;
        }
        k++;
        if (x.s1 <= cursor)
            return (size_t)-1;
        cursor = x.s1;
    }
    return k;
}

// k_hb_pack on the host: sizes as k_hb_sizes gives them (ok[i] = 0: the
// stream failed), their exclusive scan, then every tile of the grid and every
// thread of the workgroup.  count[p] = how often packed byte p was written,
// stream[p] / src[p] = from which stream and which of its bytes.  offs: n + 1
// values out.  Returns the packed total (count, stream and src hold at least
// the sum of the lengths rounded up to 16 each).
uint64_t t_pack(const uint64_t *lens, const uint8_t *ok, uint32_t n,
                uint32_t grid, uint64_t *offs, uint32_t *count,
                uint32_t *stream, uint64_t *src)
{
    uint64_t total = 0;
    for (uint32_t i = 0; i < n; i++) {
        offs[i] = total;
        total += ok[i] ? hb_align(lens[i]) : 0;
    }
    offs[n] = total;
    const uint64_t tiles = (total + kHbTile - 1) / kHbTile;
    for (uint32_t block = 0; block < grid; block++)
        for (uint64_t t = block; t < tiles; t += grid) {
            const HbTile x = hb_tile(offs, n, total, t);
            for (uint32_t thread = 0; thread < kHbTile / kHbUnit; thread++) {
                const uint64_t p = x.start + (uint64_t)kHbUnit * thread;
                if (p > x.last)
                    continue;
                const HbUnit u = hb_unit(offs, lens, x.s_lo, x.s_hi, p);
                for (uint32_t b = 0; b < u.bytes; b++) {
                    count[p + b]++;
                    stream[p + b] = u.stream;
                    src[p + b] = u.src_off + b;
                }
            }
        }
    return total;
}

} // extern "C"
