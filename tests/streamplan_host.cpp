// The long-stream decoder's plan (rust-snappy_amd/csrc/snapmi_streamplan.hpp)
// behind a C ABI for tests/test_streamplan_cpu.py: a plan of n streams is
// made, its totals and every stream's slot are read back as numbers.
#include <vector>

#include "../rust-snappy_amd/csrc/snapmi_streamplan.hpp"

using namespace snapmi;

static StreamPlan plan;
static std::vector<StreamSlot> slots;
static std::vector<uint32_t> pre;

extern "C" {
uint32_t t_seg_log2(uint32_t forced, uint64_t long_bytes)
{
    return stream_seg_log2(forced, long_bytes);
}
uint32_t t_scan_segs(uint32_t forced, uint64_t nseg)
{
    return stream_scan_segs(forced, nseg);
}
uint64_t t_lone_bound(uint64_t in_len, uint64_t out_cap)
{
    return lone_stream_bound(in_len, out_cap);
}
// is the stream worth its pieces (the route of every scalar decode and of
// every small batch)
int t_long_stream_rule(uint64_t len, uint64_t dl, uint64_t min_len)
{
    return long_stream_rule(len, dl, min_len);
}
// what the library passes plan_streams as desc_size
uint64_t t_desc_size(void) { return sizeof(StreamArgs); }
// the constants: kSeg, kEntry, kSegPerSuper, kCutSegs, kScanSegs, kScanFill,
// kStreamChunk, kPre
void t_constants(uint64_t *out)
{
    const uint64_t c[] = {kSeg, kEntry, kSegPerSuper, kCutSegs, kScanSegs,
                          kScanFill, kStreamChunk, kPre};
    for (size_t i = 0; i < sizeof c / sizeof c[0]; i++)
        out[i] = c[i];
}
// plans n streams (in_len[j], bound[j]); returns plan.fits
int t_plan(uint32_t n, const uint64_t *in_len, const uint64_t *bound,
           int lone, uint32_t forced_seg_log2, uint32_t forced_scan_segs,
           uint64_t desc_size)
{
    slots.assign(n, StreamSlot{});
    for (uint32_t j = 0; j < n; j++) {
        slots[j].in_len = in_len[j];
        slots[j].bound = bound[j];
    }
    pre.assign((size_t)kPre * (n + 1), 0xDEADBEEF);
    plan = plan_streams(slots.data(), n, lone != 0, forced_seg_log2,
                        forced_scan_segs, desc_size, pre.data());
    return plan.fits;
}
// seg_log2, scan_segs, grid[kPre], e_off, e_bytes, t_bytes, pieces, c_in,
// c_inlen, c_out, c_cap, c_outlen, c_err, c_mode, d_bytes, pre_off,
// desc_bytes
void t_totals(uint64_t *out)
{
    size_t i = 0;
    out[i++] = plan.seg_log2;
    out[i++] = plan.scan_segs;
    for (int k = 0; k < kPre; k++)
        out[i++] = plan.grid[k];
    const size_t v[] = {plan.e_off, plan.e_bytes, plan.t_bytes, plan.pieces,
                        plan.c_in, plan.c_inlen, plan.c_out, plan.c_cap,
                        plan.c_outlen, plan.c_err, plan.c_mode, plan.d_bytes,
                        plan.pre_off, plan.desc_bytes};
    for (size_t x : v)
        out[i++] = x;
}
// nseg, nsuper, nsuper3, kmax, meta, e1, e2, e3, s1, s2, s3, cuts, entry of
// every stream (13 each)
void t_slots(uint64_t *out)
{
    for (const StreamSlot &g : slots) {
        const uint64_t v[] = {g.nseg, g.nsuper, g.nsuper3, g.kmax, g.meta,
                              g.e1, g.e2, g.e3, g.s1, g.s2, g.s3, g.cuts,
                              g.entry};
        for (uint64_t x : v)
            *out++ = x;
    }
}
// the prefixes, [kPre][n + 1]
void t_pre(uint32_t *out)
{
    for (size_t i = 0; i < pre.size(); i++)
        out[i] = pre[i];
}
}
