// The compressor's routing (rust-snappy_amd/csrc/snapmi_route.hpp) behind a
// C ABI for tests/test_route_cpu.py: options are set by name, a route is
// computed, its fields are read by name.
#include <cstring>

#include "../rust-snappy_amd/csrc/snapmi_route.hpp"

using namespace snapmi;

static RouteOptions opts;
static CompressRoute route;

#define FIELDS(X)                                                             \
    X(compress_mode) X(lds_order_ok) X(num_cus) X(lane_min_blocks)            \
    X(lane_segment_blocks) X(lane_waves_per_cu) X(lane_max_waves)             \
    X(lane_coresident) X(lane_coresident_min_blocks) X(small_table_kernel)    \
    X(small_table_min_blocks) X(small_batch_kernel) X(span_kernel)            \
    X(span_schedule) X(both_wave_cus) X(match_kernel) X(lane_speculate)       \
    X(lane_speculate_max_blocks) X(lane_overlap_encode)                       \
    X(tiny_stream_kernel) X(small_stream_kernel)

#define ROUTE_FIELDS(X)                                                       \
    X(window_grid) X(window_beside) X(sched) X(tokens) X(small_grid)          \
    X(nb_big) X(direct) X(post_ratio) X(seg_blocks) X(lanes) X(stage_waves)

extern "C" {
// 0, or -1 for a name the options do not have
int t_set(const char *name, int64_t v)
{
#define SET(f)                                                                \
    if (strcmp(name, #f) == 0) {                                              \
        opts.f = (decltype(opts.f))v;                                         \
        return 0;                                                             \
    }
    FIELDS(SET)
#undef SET
    return -1;
}
void t_route(uint64_t blocks, uint64_t cnt8, int spans_hint)
{
    route = compress_route(opts, blocks, cnt8, spans_hint != 0);
}
// a field of the last route (window and match: their enumerators' order)
int64_t t_get(const char *name)
{
#define GET(f)                                                                \
    if (strcmp(name, #f) == 0)                                                \
        return (int64_t)route.f;
    ROUTE_FIELDS(GET)
#undef GET
    if (strcmp(name, "window") == 0)
        return (int64_t)route.window;
    if (strcmp(name, "match") == 0)
        return (int64_t)route.match;
    return -1;
}
const char *t_last_kernel() { return route.last_kernel; }
uint32_t t_match_grid(uint64_t count) { return match_grid(opts, route, count); }
// the last route's segment [lo, hi): mid, spec, redo_grid
void t_segment(uint64_t lo, uint64_t hi, uint64_t *out)
{
    const Segment g = segment(opts, route, lo, hi);
    out[0] = g.mid;
    out[1] = g.spec;
    out[2] = g.redo_grid;
}
uint32_t t_prepare_lanes(uint64_t blocks) { return prepare_lanes(opts, blocks); }
uint64_t t_small_stream_limit() { return small_stream_limit(opts); }
}
