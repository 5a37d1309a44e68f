// snapmi_hostpipe.hpp -- private: the three-slot staging pipeline of the
// host-buffer calls (snapmi_hostpipe.hip owns it; snapmi_hostbatch.hip shares
// it).
//
// A batch is cut into slices; slice i+1 is on its way to the device (copy
// stream 1) while the kernels of slice i run (the context's stream) and the
// result of slice i-1 goes back to the host (copy stream 2): PCIe is full
// duplex, and the three legs of a batch cost about the same (a 4 GiB corpus
// batch: 78 ms in, 60 ms of kernels, 39 ms out - 177 ms one after the other).
// Three slots of device staging, so that none of the three legs waits for a
// buffer of the other two.  Host memory from snapmi_host_alloc (pinned) is
// what makes the copies asynchronous; pageable memory works, one leg at a
// time.
#pragma once

#include "snapmi_ctx.hpp"
#include "snapmi_launch.hpp" // pin_reserve and the codec's launchers

namespace snapmi {

constexpr int kSlots = 3;

struct PipeSlot {
    ScratchDev in, out, desc; // desc: u64 len | snapmi_error | index...
    hipEvent_t ev_h2d = nullptr, ev_k = nullptr, ev_d2h = nullptr;
    struct Result {
        uint64_t len;
        snapmi_error e;
    } *h_res = nullptr;            // pinned
    uint64_t *h_off = nullptr;     // pinned: chunk offsets of the slice
    size_t h_off_cap = 0;
    // the host-memory batch calls (snapmi_hostbatch.hip): the slice's results
    // and packed output on the device; pinned staging of what goes in
    // (descriptors + packed inputs) and of what comes home
    ScratchDev home;
    ScratchPin hb_in, hb_home;
};

} // namespace snapmi

struct snapmi_host_pipe {
    hipStream_t s_in = nullptr, s_out = nullptr;
    snapmi::PipeSlot slot[snapmi::kSlots];
};

namespace snapmi {

// Every exit of a host-buffer call that comes after its first asynchronous
// operation goes through this: an early return (a failed allocation, a
// capacity check, an error of the codec call) must not hand the caller's
// buffers back while copies of earlier slices still read or write them, and
// the next call relies on "the previous call ended with its streams idle".
struct PipeDrain {
    snapmi_ctx *ctx;
    snapmi_host_pipe *pipe;
    bool armed = true;
    ~PipeDrain()
    {
        if (!armed)
            return;
        (void)hipStreamSynchronize(pipe->s_in);
        (void)hipStreamSynchronize(ctx->stream);
        (void)hipStreamSynchronize(pipe->s_out);
    }
};

// snapmi_hostpipe.hip
// the context's pipe, made on first use
int host_pipe(snapmi_ctx *ctx, snapmi_host_pipe **out);
// a slot's device buffer grows only when nothing of the slot is in flight
int slot_reserve(snapmi_ctx *ctx, DevBuf &b, size_t bytes);
// n bytes of device memory into pinned, device-mapped host memory on `st`:
// by k_to_host (16-byte stores over the link) or by hipMemcpyAsync
int pipe_copy_home(snapmi_ctx *ctx, hipStream_t st, uint8_t *h_dst,
                   const void *d_src, uint64_t n, bool by_kernel);

} // namespace snapmi
