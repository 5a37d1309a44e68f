// Host build of the no-wait decode's rules (csrc/snapmi_framewalk.hpp) for
// tests/test_frame_nowait_cpu.py: the side-index check the index kernel runs
// entry by entry, the sequential walk under the caller's bound, and the rule
// that says which front decided, whether the bound was exceeded and which
// records of the chunk table are padding - chained the way
// snapmi_frame_decompress_ex enqueues the fronts.
#include <stdint.h>
#include <stddef.h>

#include <vector>

#include "../rust-snappy_amd/csrc/snapmi_framewalk.hpp"

using namespace snapmi;

extern "C" {

uint32_t t_flag_nowait(void) { return SNAPMI_FRAME_NO_WAIT; }

// The side index alone: 1 when every entry and the start pass, 0 when the
// stream goes to the walk.  good[i] (n entries) = entry i's own answer;
// no index entry behind index[n] is read.
int t_index_front(const uint8_t *in, uint64_t len, uint32_t flags,
                  const uint64_t *index, uint32_t n, uint8_t *good)
{
    bool ok = frame_index_start(in, len, flags, n);
    for (uint32_t i = 0; i < n; i++) {
        FrameChunk c;
        const bool g = frame_index_entry(in, len, flags, index, n, i, c);
        good[i] = g;
        ok = ok && g;
        // a failed entry leaves a record that decodes to nothing
        if (!g && (c.type != 0xFF || c.payload_len != 0 || c.payload_off != 0))
            return -1;
        if (g && (c.payload_off != index[i] + 8 ||
                  c.payload_off + c.payload_len != index[i + 1]))
            return -1;
    }
    return ok;
}

// The chain of one no-wait decode.  index: NULL or n_chunks + 1 entries;
// parallel: 0 the parallel walk is not enqueued, 1 it is and hands the stream
// on, 2 it is and decides with parallel_found data chunks (the kernels of that
// front are device code: its outcome is the caller's to state).
// out: front, exceeded, chunks, pad_lo, found, the table's records that are
// chunks of the stream, those that decode to nothing, verdict kind, a, b.
void t_nowait(const uint8_t *in, uint64_t len, uint32_t flags,
              const uint8_t *stale, const uint64_t *index, uint32_t n_chunks,
              uint32_t parallel, uint32_t parallel_found, uint64_t *out)
{
    std::vector<FrameChunk> table(n_chunks);
    for (auto &c : table) // what an earlier call left: anything
        c.type = 7, c.payload_off = ~0ull, c.payload_len = 99;
    uint32_t first = kFrontWalk, handed_on = 0, found = 0;
    if (index) {
        first = kFrontIndex;
        found = n_chunks;
        handed_on = frame_index_start(in, len, flags, n_chunks) ? 0 : 1;
        for (uint32_t i = 0; i < n_chunks; i++)
            if (!frame_index_entry(in, len, flags, index, n_chunks, i,
                                   table[i]))
                handed_on = 1;
    } else if (parallel) {
        first = kFrontParallel;
        handed_on = parallel == 2 ? 0 : 2;
        found = parallel == 2 ? parallel_found : 0;
        if (parallel == 2 && found <= n_chunks) // (k_fw_emit)
            for (uint32_t i = 0; i < found; i++)
                table[i].type = 0, table[i].payload_off = 8,
                table[i].payload_len = 0;
    }
    bool walk_ran = false;
    snapmi_error serr = frame_err(SNAPMI_OK, 0, 0);
    if (first == kFrontWalk || !frame_front_decided(handed_on)) {
        walk_ran = first != kFrontWalk;
        serr = frame_walk(in, len, flags & SNAPMI_FRAME_CONTINUATION, stale,
                          found, [&](uint32_t k, const FrameChunk &c) {
                              if (k < n_chunks)
                                  table[k] = c;
                          });
    }
    const FrameNowait x = frame_nowait_rule(first, walk_ran, found, n_chunks);
    for (uint32_t t = x.pad_lo; t < n_chunks; t++)
        table[t] = frame_no_chunk();
    if (x.exceeded)
        serr = frame_nowait_exceeded(found, n_chunks);
    uint64_t chunks = 0, nothing = 0;
    for (uint32_t t = 0; t < n_chunks; t++) {
        snapmi_error e;
        const FrameChunk &c = table[t];
        if (c.type <= 1 && c.payload_off + c.payload_len <= len)
            chunks++;
        else if (frame_chunk_len((const uint8_t *)nullptr, c, e) == 0 &&
                 c.payload_len == 0)
            nothing++; // (no payload byte was read: the pointer is NULL)
    }
    out[0] = x.front;
    out[1] = x.exceeded;
    out[2] = x.chunks;
    out[3] = x.pad_lo;
    out[4] = found;
    out[5] = chunks;
    out[6] = nothing;
    out[7] = (uint64_t)(int64_t)serr.kind;
    out[8] = serr.a;
    out[9] = serr.b;
}

} // extern "C"
