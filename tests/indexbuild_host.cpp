// Host build of csrc/snapmi_blockindex.hpp for tests/test_index_build_cpu.py:
// bi_build, the sequential definition of snapmi_build_block_index, as the
// host code and the kernels compile it.
#include <stdint.h>
#include <stddef.h>

#include "../rust-snappy_amd/csrc/snapmi_blockindex.hpp"

using namespace snapmi;

extern "C" {

// e: bi_entries(dlen) entries; returns the verdict (1 .. 4)
int t_build(const uint8_t *in, uint64_t in_len, uint64_t dlen, uint64_t *e)
{
    return bi_build(in, in_len, dlen, e);
}

int t_status(int which)
{
    const int v[4] = {kBiBuilt, kBiUnaligned, kBiCorrupt, kBiMissized};
    return v[which];
}

} // extern "C"
