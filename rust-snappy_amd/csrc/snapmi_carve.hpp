// snapmi_carve.hpp -- one buffer, many arrays: the frame layer's scratch
// buffers (fb_streams, fb_chunks, fr_desc, fr_crc) each hold a list of arrays,
// one behind the other, every one on a 16-byte boundary.  A layout function
// names each array once, with its count, through a Carver; the host runs it
// twice - without a base for the size to reserve, then on the buffer for the
// addresses - so the size and the places come from the same statements.
// Host only, no HIP (tests/test_carve_cpu.py).
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace snapmi {

class Carver {
  public:
    // measuring: every take() hands out nullptr, bytes() is what to reserve
    Carver() : base_(nullptr) {}
    // placing: `base` must be 16-byte aligned (hipMalloc's are 256-aligned)
    explicit Carver(void *base) : base_((uint8_t *)base) {}

    // the next array: `count` elements of T on a 16-byte boundary; an array
    // of no elements takes no room
    template <class T> T *take(size_t count)
    {
        const size_t at = (off_ + 15) & ~(size_t)15;
        if (count)
            off_ = at + count * sizeof(T);
        return base_ ? (T *)(base_ + at) : nullptr;
    }
    // what the arrays so far take, up to the next boundary: where an array
    // of no elements behind them would lie
    size_t bytes() const { return (off_ + 15) & ~(size_t)15; }

  private:
    uint8_t *base_;
    size_t off_ = 0;
};

} // namespace snapmi
