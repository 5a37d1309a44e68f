// The compressor's routing (rust-snappy_amd/csrc/snapmi_route.hpp) behind a
// C ABI for tests/test_route_cpu.py: options are set by name through the
// library's own table (snapmi_options.hpp), a route is computed, its fields
// are read by name.
#include <cstring>

#include "../rust-snappy_amd/csrc/snapmi_route.hpp"

using namespace snapmi;

static Options opts; // snapmi_options.hpp's defaults
static RouteDevice dev = {false, 0};
static CompressRoute route;

#define ROUTE_FIELDS(X)                                                       \
    X(window_grid) X(window_beside) X(sched) X(tokens) X(small_grid)          \
    X(nb_big) X(direct) X(post_ratio) X(seg_blocks) X(lanes) X(stage_waves)

extern "C" {
// back to the defaults, on a device nothing is known of
void t_reset()
{
    opts = Options{};
    dev = {false, 0};
}
// 0, or -1 for a name or a value the options do not have: the two facts of
// the device, then what either setter of the test build accepts
int t_set(const char *name, int64_t v)
{
    if (strcmp(name, "lds_order_ok") == 0) {
        dev.lds_order_ok = v != 0;
        return 0;
    }
    if (strcmp(name, "num_cus") == 0) {
        dev.num_cus = (uint32_t)v;
        return 0;
    }
    const OptionDesc *d = find_named(kOptions, name);
    return d && option_set(opts, name, v, d->test_only, true) ==
                    OptionSet::accepted
               ? 0
               : -1;
}
// an option's default: its value in a fresh Options
int64_t t_default(const char *name)
{
    const OptionDesc *d = find_named(kOptions, name);
    return d && d->load ? d->load(Options{}) : -1;
}
void t_route(uint64_t blocks, uint64_t cnt8, int spans_hint)
{
    route = compress_route(opts, dev, blocks, cnt8, spans_hint != 0);
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
uint32_t t_match_grid(uint64_t count) { return match_grid(dev, route, count); }
// the last route's segment [lo, hi): mid, spec, redo_grid
void t_segment(uint64_t lo, uint64_t hi, uint64_t *out)
{
    const Segment g = segment(opts, dev, route, lo, hi);
    out[0] = g.mid;
    out[1] = g.spec;
    out[2] = g.redo_grid;
}
uint32_t t_prepare_lanes(uint64_t blocks)
{
    return prepare_lanes(opts, dev, blocks);
}
uint64_t t_small_stream_limit() { return small_stream_limit(opts); }
}
