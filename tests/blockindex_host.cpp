// Host build of csrc/snapmi_blockindex.hpp for tests/test_block_index_cpu.py:
// the entry count, the rule that says whether a stream is indexed, the piece
// ranges and the entry -> stream search, as the kernels call them.
#include <stdint.h>
#include <stddef.h>

#include "../rust-snappy_amd/csrc/snapmi_blockindex.hpp"

using namespace snapmi;

extern "C" {

uint64_t t_block(void) { return kBiBlock; }
uint64_t t_entries(uint64_t len) { return bi_entries(len); }

// header bytes (0: none), *dlen its value
uint32_t t_header(const uint8_t *in, uint64_t in_len, uint64_t *dlen)
{
    return bi_header(in, in_len, dlen);
}

int t_indexed(const uint8_t *in, uint64_t in_len, uint64_t cap,
              const uint64_t *index, uint64_t first, uint64_t next,
              uint64_t index_entries)
{
    return bi_stream_indexed(in, in_len, cap, index, first, next,
                             index_entries)
               ? 1
               : 0;
}

// out4: in_off, in_len, out_off, out_len
void t_piece(const uint64_t *e, uint64_t dlen, uint64_t k, uint64_t *out4)
{
    const BiPiece p = bi_piece(e, dlen, k);
    out4[0] = p.in_off;
    out4[1] = p.in_len;
    out4[2] = p.out_off;
    out4[3] = p.out_len;
}

uint32_t t_find(const uint64_t *first, uint32_t n, uint64_t e)
{
    return bi_find_stream(first, n, e);
}

} // extern "C"
