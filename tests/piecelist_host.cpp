// Stand-alone host build of csrc/snapmi_piecelist.hpp (and of plan_streams of
// csrc/snapmi_streamplan.hpp, which sizes sd_desc with it) for
// tests/test_piecelist_cpu.py: one slot count P per line of standard input,
// one line of answer each:
//   slot_bytes  c_in c_inlen c_out c_cap c_outlen c_err c_mode total   (offsets)
//   the same seven as piece_list() lays them over a 256-byte aligned base
//   base % 256
//   c_in c_inlen c_out c_cap c_outlen c_err c_mode d_bytes of a plan of P
//   pieces - or eight times 18446744073709551615 when no plan has P pieces
//   (a stream has two at the least)
// The first and the last slot of every array are written, so that a build
// with -fsanitize=address,undefined (it has a main of its own and runs as it
// is) sees a slab that is sized short.
#include <inttypes.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../rust-snappy_amd/csrc/snapmi_streamplan.hpp"

using namespace snapmi;

// (complete here: the header only names it)
struct snapmi_error {
    uint8_t bytes[kPieceErrBytes];
};

int main()
{
    unsigned long long in;
    while (scanf("%llu", &in) == 1) {
        const size_t P = (size_t)in;
        const PieceOffsets o = piece_offsets(P);
        printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu", kPieceSlotBytes, o.c_in,
               o.c_inlen, o.c_out, o.c_cap, o.c_outlen, o.c_err, o.c_mode,
               o.total);
        void *mem = nullptr;
        if (posix_memalign(&mem, 256, o.total))
            return 3;
        uint8_t *const base = (uint8_t *)mem;
        const PieceList l = piece_list(base, P);
        if (P) {
            for (size_t k : {(size_t)0, P - 1}) {
                l.c_in[k] = nullptr;
                l.c_inlen[k] = 1;
                l.c_out[k] = nullptr;
                l.c_cap[k] = 2;
                l.c_outlen[k] = 3;
                memset(&l.c_err[k], 4, sizeof(snapmi_error));
                l.c_mode[k] = 5;
            }
        }
        const uint8_t *at[] = {(const uint8_t *)l.c_in,
                               (const uint8_t *)l.c_inlen,
                               (const uint8_t *)l.c_out,
                               (const uint8_t *)l.c_cap,
                               (const uint8_t *)l.c_outlen,
                               (const uint8_t *)l.c_err,
                               (const uint8_t *)l.c_mode};
        for (const uint8_t *p : at)
            printf(" %zu", (size_t)(p - base));
        printf(" %zu", (size_t)((uintptr_t)base % 256));
        free(base);

        // a plan of P pieces: one stream of P - 2 whole chunks of output
        if (P == 0 || P >= 2) {
            std::vector<StreamSlot> slot(P ? 1 : 0);
            std::vector<uint32_t> pre((size_t)kPre * (slot.size() + 1));
            if (P) {
                slot[0].in_len = 1000;
                slot[0].bound = (uint64_t)(P - 2) * kStreamChunk;
            }
            const StreamPlan p =
                plan_streams(slot.data(), (uint32_t)slot.size(), false, 0, 0,
                             256, pre.data());
            if (!p.fits || p.pieces != P)
                return 4;
            printf(" %zu %zu %zu %zu %zu %zu %zu %zu\n", p.c_in, p.c_inlen,
                   p.c_out, p.c_cap, p.c_outlen, p.c_err, p.c_mode, p.d_bytes);
        } else {
            for (int k = 0; k < 8; k++)
                printf(" %" PRIu64, ~(uint64_t)0);
            printf("\n");
        }
    }
    return 0;
}
