// The option table and the info names (rust-snappy_amd/csrc/
// snapmi_options.hpp) behind a C ABI for tests/test_options_cpu.py and the
// tests that ask whether a name is accepted: the tables are walked by index,
// a value is tried the way either setter of either build would try it.
#include <iterator>

#include "../rust-snappy_amd/csrc/snapmi_options.hpp"

using namespace snapmi;

extern "C" {
uint64_t t_option_count() { return std::size(kOptions); }
const char *t_option_name(uint64_t i) { return kOptions[i].name; }
int t_option_test_only(uint64_t i) { return kOptions[i].test_only; }
// 1: the option is stored in a field (t_option_default reads it)
int t_option_has_field(uint64_t i) { return kOptions[i].load != nullptr; }
int64_t t_option_default(uint64_t i) { return kOptions[i].load(Options{}); }
// -1: no option of that name
int64_t t_option_index(const char *name)
{
    const OptionDesc *d = find_named(kOptions, name);
    return d ? d - kOptions : -1;
}
// option_set on a fresh Options: 0 accepted, 1 unknown name, 2 refused
// value; *stored: what the field then holds (untouched without a field)
int t_option_try(const char *name, int64_t value, int test_entry_point,
                 int test_build, int64_t *stored)
{
    Options o;
    const OptionSet r =
        option_set(o, name, value, test_entry_point != 0, test_build != 0);
    if (r == OptionSet::accepted && find_named(kOptions, name)->load)
        *stored = find_named(kOptions, name)->load(o);
    return (int)r;
}

uint64_t t_info_count() { return std::size(kInfoNames); }
const char *t_info_name(uint64_t i) { return kInfoNames[i].name; }
int t_info_test_only(uint64_t i) { return kInfoNames[i].test_only; }
}
