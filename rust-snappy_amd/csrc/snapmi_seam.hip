// snapmi_seam.hip -- the libsnappy C API over a process-wide pool of
// contexts: concurrent calls are combined into batches.
#include <hip/hip_runtime.h>

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "snapmi.h"
#include "snapmi_test.h"
#include "snapmi_ctx.hpp"
#include "snapmi_launch.hpp"
#include "snapmi_device.hpp"
#include "snapmi_kernels.hpp"

using namespace snapmi;

extern "C" {

// ----------------------------------------------------------------------
// libsnappy C API (snappy-c.h), as bound by the reference's snappy-cpp
// crate.  The reference's wrappers are stateless and may be called from any
// number of threads at once (snappy-cpp/src/lib.rs:13-64), so these calls
// share a small process-wide pool of contexts on device SNAPMI_DEVICE
// (default 0; created on demand, up to SNAPMI_SEAM_CONTEXTS, default 2).
//
// Round 5: concurrent calls are COMBINED.  One call is ~1.5 ms of a lone
// wavefront per block whatever else the GPU does, so eight callers on eight
// streams got 3.3-3.8x the rate of one (round 4) - but a batch of sixteen such
// streams takes about as long as one.  A caller stages its input in pinned
// memory of its own thread, queues a request and either finds it done by
// another caller or becomes a leader: it takes a context, waits a few
// microseconds for requests that are just arriving, takes every queued
// request of its kind and runs them as ONE snapmi_compress_batch /
// snapmi_decompress_batch - per-request copies in, one launch, per-request
// copies out, one wait.  Every caller then moves its own bytes from its
// pinned buffer to the buffer it was given.  Results and errors are per
// stream, exactly those of the batch call.  Inputs of more than kPinStage
// bytes go one by one, as before.
// ----------------------------------------------------------------------
namespace {
struct SeamPool {
    std::mutex mu;
    std::condition_variable cv;
    std::vector<snapmi_ctx *> idle;
    size_t created = 0, cap = 0;
    bool broken = false; // a context could not be created: do not retry

    // (mu held) a context if one is idle or may still be created; *wait =
    // whether one will come back
    snapmi_ctx *checkout_locked(std::unique_lock<std::mutex> &lock,
                                bool block, bool *none)
    {
        *none = false;
        if (cap == 0) {
            // (two: one batch runs while the next one gathers - with more
            // contexts the callers spread over more, smaller batches: 16
            // callers on alice29.txt 1 240 / 1 060 / 740 MB/s with 2 / 4 / 8,
            // profiles/r5_seam_sweep.txt)
            cap = 2;
            if (const char *e = getenv("SNAPMI_SEAM_CONTEXTS"))
                cap = (size_t)(atoi(e) < 1 ? 1 : atoi(e));
        }
        for (;;) {
            if (!idle.empty()) {
                snapmi_ctx *c = idle.back();
                idle.pop_back();
                return c;
            }
            if (created < cap && !broken) {
                created++; // reserved: created outside the lock
                lock.unlock();
                int dev = 0;
                if (const char *e = getenv("SNAPMI_DEVICE"))
                    dev = atoi(e);
                snapmi_ctx *c = nullptr;
                const bool ok = snapmi_ctx_create(dev, nullptr, &c) == SNAPMI_OK;
                lock.lock();
                if (ok)
                    return c;
                created--;
                broken = true; // (snapmi_ctx_create has printed why)
                cv.notify_all();
            }
            if (created == 0) {
                *none = true; // no context and none can be made
                return nullptr;
            }
            if (!block)
                return nullptr;
            cv.wait(lock);
        }
    }
    snapmi_ctx *checkout()
    {
        std::unique_lock<std::mutex> lock(mu);
        bool none;
        return checkout_locked(lock, true, &none);
    }
    void give_back(snapmi_ctx *c)
    {
        {
            std::lock_guard<std::mutex> lock(mu);
            idle.push_back(c);
        }
        cv.notify_all();
    }
};
SeamPool g_pool;

struct SeamLease {
    snapmi_ctx *ctx;
    SeamLease() : ctx(g_pool.checkout()) {}
    ~SeamLease()
    {
        if (ctx)
            g_pool.give_back(ctx);
    }
};

// set by an atexit handler: the process is leaving, the HIP runtime with it
std::atomic<bool> g_seam_exiting{false};
struct SeamExitHook {
    SeamExitHook()
    {
        atexit([] { g_seam_exiting.store(true, std::memory_order_release); });
    }
} g_seam_exit_hook;

// pinned staging of the calling thread (at most 2 MiB kept between calls,
// freed with the thread)
struct ThreadPin {
    void *p = nullptr;
    size_t cap = 0;
    bool reserve(size_t bytes)
    {
        if (bytes <= cap)
            return true;
        if (p)
            (void)hipHostFree(p);
        p = nullptr;
        cap = 0;
        const size_t want = bytes + bytes / 4 + 4096;
        if (hipHostMalloc(&p, want, hipHostMallocDefault) != hipSuccess) {
            (void)hipGetLastError();
            p = nullptr;
            return false;
        }
        cap = want;
        return true;
    }
    // a call that needed a large buffer does not leave it with the thread
    // for good: above kKeep the buffer goes back once the call is over
    static constexpr size_t kKeep = (size_t)2 << 20;
    void trim()
    {
        if (cap > kKeep) {
            (void)hipHostFree(p);
            p = nullptr;
            cap = 0;
        }
    }
    ~ThreadPin()
    {
        // (a thread that ends while the process is leaving may find the HIP
        // runtime gone: its own teardown frees pinned memory then, and a
        // call into it would not come back)
        if (p && !g_seam_exiting.load(std::memory_order_acquire))
            (void)hipHostFree(p);
    }
};
thread_local ThreadPin tl_pin_in, tl_pin_out;

struct SeamReq {
    bool compress;
    size_t in_len, out_cap; // the caller's
    size_t dev_out;         // bytes the device may write = bytes coming back
    const uint8_t *pin_in;  // the caller's pinned copy of its input
    uint8_t *pin_out;       // ... and room for dev_out bytes of result
    int state;              // 0 queued, 1 taken by a leader, 2 done
    int rc;
    size_t written;
    snapmi_error err;
};

// The single-launch path of a lone small call (round 6): a request of under
// 256 bytes (compress: input; uncompress: compressed bytes, at most 256 of
// output) that has no company runs as ONE kernel whose descriptor, input and
// output lie in pinned host memory - the caller's staging buffers, which the
// device reaches over the link - and whose end the host sees by polling a
// word of that memory: no copy commands, no plan kernel, no stream
// synchronisation (round 5: two copies each way, two to three kernels and a
// hipStreamSynchronize, ~80 us for 200 bytes).  The reference's seam is a
// plain function call (snappy-cpp/src/lib.rs:13-64); this is as close as a
// device gets.  Returns false when it cannot run (the batch path takes over).
struct SeamTinyBlock {  // in ctx->pin_desc
    uint64_t in_ptr, in_len, out_ptr, out_cap, out_len;
    snapmi_error err;
    uint32_t order0;         // DecompressArgs::order: stream 0
    uint32_t bucket_pos[66]; // (unused by the kernel; room the args point at)
    uint32_t done;
};

bool seam_tiny(snapmi_ctx *ctx, SeamReq *r)
{
    if (r->in_len == 0 || r->in_len >= kTinyCompress)
        return false;
    if (r->compress ? !ctx->tiny_stream_kernel : r->dev_out > 256)
        return false;
    if (pin_reserve(ctx, ctx->pin_desc, sizeof(SeamTinyBlock) + 64) !=
        SNAPMI_OK)
        return false;
    SeamTinyBlock *h = (SeamTinyBlock *)ctx->pin_desc.p;
    void *d_blk = nullptr, *d_in = nullptr, *d_out = nullptr;
    if (hipHostGetDevicePointer(&d_blk, h, 0) != hipSuccess ||
        hipHostGetDevicePointer(&d_in, (void *)r->pin_in, 0) != hipSuccess ||
        hipHostGetDevicePointer(&d_out, r->pin_out, 0) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    SeamTinyBlock *d = (SeamTinyBlock *)d_blk;
    const uint32_t seq = ++ctx->seam_seq ? ctx->seam_seq : ++ctx->seam_seq;
    h->in_ptr = (uint64_t)(uintptr_t)d_in;
    h->in_len = r->in_len;
    h->out_ptr = (uint64_t)(uintptr_t)d_out;
    h->out_cap = r->out_cap < r->dev_out ? r->out_cap : r->dev_out;
    h->out_len = 0;
    memset(&h->err, 0, sizeof h->err);
    h->order0 = 0;
    h->done = 0;
    std::atomic_thread_fence(std::memory_order_seq_cst);
    if (r->compress) {
        hipLaunchKernelGGL(k_seam_compress_tiny, dim3(1), dim3(64), 0,
                           ctx->stream, (const uint8_t *)d_in,
                           (uint32_t)r->in_len, (uint8_t *)d_out,
                           (unsigned long long *)&d->out_len, &d->done, seq);
    } else {
        DecompressArgs a;
        memset(&a, 0, sizeof a);
        a.in_ptrs = (const void *const *)&d->in_ptr;
        a.in_lens = &d->in_len;
        a.out_ptrs = (void *const *)&d->out_ptr;
        a.out_caps = &d->out_cap;
        a.out_lens = &d->out_len;
        a.errs = &d->err;
        a.n_streams = 1;
        a.order = &d->order0;
        a.bucket_pos = d->bucket_pos;
        hipLaunchKernelGGL(k_seam_decompress_tiny, dim3(1), dim3(64), 0,
                           ctx->stream, a, &d->done, seq);
    }
    if (hipGetLastError() != hipSuccess)
        return false;
    // the end: the device's release store of `seq` (spin; after 2 ms of it,
    // the stream's own wait - a queue behind somebody else's work)
    volatile uint32_t *done = &h->done;
    const auto t0 = std::chrono::steady_clock::now();
    bool seen = false;
    for (uint32_t spins = 0;; spins++) {
        if (*done == seq) {
            seen = true;
            break;
        }
        if ((spins & 255) == 255 &&
            std::chrono::steady_clock::now() - t0 >
                std::chrono::milliseconds(2))
            break;
    }
    if (!seen && (hipStreamSynchronize(ctx->stream) != hipSuccess ||
                  *done != seq)) {
        (void)hipGetLastError();
        r->rc = SNAPMI_E_DEVICE;
        r->written = 0;
        memset(&r->err, 0, sizeof r->err);
        r->err.kind = SNAPMI_E_DEVICE;
        return true;
    }
    std::atomic_thread_fence(std::memory_order_seq_cst);
    r->err = h->err;
    r->rc = r->compress ? SNAPMI_OK : h->err.kind;
    r->written = r->rc == SNAPMI_OK ? (size_t)h->out_len : 0;
    if (r->written > r->dev_out) {
        r->rc = SNAPMI_E_DEVICE;
        r->written = 0;
    }
    return true;
}

// one batch of requests of one kind on `ctx` (no lock held)
void seam_execute(snapmi_ctx *ctx, const std::vector<SeamReq *> &batch)
{
    const size_t n = batch.size();
    const bool compress = batch[0]->compress;
    if (n == 1 && hipSetDevice(ctx->device) == hipSuccess &&
        seam_tiny(ctx, batch[0]))
        return;
    auto fail_all = [&](int rc) {
        for (SeamReq *r : batch) {
            r->rc = rc;
            r->written = 0;
            memset(&r->err, 0, sizeof r->err);
            r->err.kind = rc;
        }
    };
    if (hipSetDevice(ctx->device) != hipSuccess) {
        (void)hipGetLastError();
        return fail_all(SNAPMI_E_DEVICE);
    }
    // device slabs: inputs and outputs back to back, 16-byte aligned
    std::vector<size_t> in_off(n), out_off(n);
    size_t in_total = 0, out_total = 0;
    for (size_t i = 0; i < n; i++) {
        in_off[i] = in_total;
        in_total += (batch[i]->in_len + 16 + 15) & ~(size_t)15;
        out_off[i] = out_total;
        out_total += (batch[i]->dev_out + 64 + 15) & ~(size_t)15;
    }
    // descriptors, structure of arrays: in_ptrs, in_lens, out_ptrs, out_caps,
    // out_lens (8 bytes each), errs (32)
    const size_t desc_bytes = n * (5 * 8 + sizeof(snapmi_error));
    int rc;
    if ((rc = reserve(ctx, ctx->st_in, in_total + 16)) ||
        (rc = reserve(ctx, ctx->st_out, out_total + 64)) ||
        (rc = reserve(ctx, ctx->st_desc, desc_bytes)) ||
        (rc = pin_reserve(ctx, ctx->pin_desc, 2 * desc_bytes)))
        return fail_all(rc);
    uint8_t *hd = (uint8_t *)ctx->pin_desc.p, *hback = hd + desc_bytes;
    uint8_t *dd = (uint8_t *)ctx->st_desc.p;
    uint64_t *h_in_ptrs = (uint64_t *)hd, *h_in_lens = h_in_ptrs + n,
             *h_out_ptrs = h_in_lens + n, *h_out_caps = h_out_ptrs + n;
    memset(hd, 0, desc_bytes);
    for (size_t i = 0; i < n; i++) {
        h_in_ptrs[i] = (uint64_t)(uintptr_t)((uint8_t *)ctx->st_in.p + in_off[i]);
        h_in_lens[i] = batch[i]->in_len;
        h_out_ptrs[i] =
            (uint64_t)(uintptr_t)((uint8_t *)ctx->st_out.p + out_off[i]);
        // (the caller's capacity was checked against what the call needs -
        // max_compress_len / the header's length - before it got here; the
        // kernels get what the request's slab holds, so that their own cap
        // checks keep them inside it)
        h_out_caps[i] = batch[i]->out_cap < batch[i]->dev_out
                            ? batch[i]->out_cap
                            : batch[i]->dev_out;
    }
    hipStream_t s = ctx->stream;
    bool ok = true;
    for (size_t i = 0; i < n && ok; i++)
        if (batch[i]->in_len)
            ok = hipMemcpyAsync((uint8_t *)ctx->st_in.p + in_off[i],
                                batch[i]->pin_in, batch[i]->in_len,
                                hipMemcpyHostToDevice, s) == hipSuccess;
    ok = ok && hipMemcpyAsync(dd, hd, desc_bytes, hipMemcpyHostToDevice, s) ==
                   hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        (void)hipStreamSynchronize(s);
        return fail_all(SNAPMI_E_DEVICE);
    }
    const void *const *d_in_ptrs = (const void *const *)dd;
    const uint64_t *d_in_lens = (const uint64_t *)(dd + 8 * n);
    void *const *d_out_ptrs = (void *const *)(dd + 16 * n);
    const uint64_t *d_out_caps = (const uint64_t *)(dd + 24 * n);
    uint64_t *d_out_lens = (uint64_t *)(dd + 32 * n);
    snapmi_error *d_errs = (snapmi_error *)(dd + 40 * n);
    if (compress)
        rc = snapmi_compress_batch(ctx, d_in_ptrs, d_in_lens, h_in_lens,
                                   d_out_ptrs, d_out_caps, d_out_lens, d_errs,
                                   n);
    else
        rc = snapmi_decompress_batch(ctx, d_in_ptrs, d_in_lens, d_out_ptrs,
                                     d_out_caps, d_out_lens, d_errs, n);
    if (rc) {
        (void)hipStreamSynchronize(s);
        return fail_all(rc);
    }
    ok = hipMemcpyAsync(hback, dd, desc_bytes, hipMemcpyDeviceToHost, s) ==
         hipSuccess;
    // the results come along in the same round trip: as much as the kernels
    // can have written (the lengths are not known to the host yet)
    for (size_t i = 0; i < n && ok; i++)
        if (batch[i]->dev_out)
            ok = hipMemcpyAsync(batch[i]->pin_out,
                                (uint8_t *)ctx->st_out.p + out_off[i],
                                batch[i]->dev_out, hipMemcpyDeviceToHost,
                                s) == hipSuccess;
    if (hipStreamSynchronize(s) != hipSuccess || !ok) {
        (void)hipGetLastError();
        return fail_all(SNAPMI_E_DEVICE);
    }
    (void)release_batch_scratch(ctx);
    const uint64_t *b_out_lens = (const uint64_t *)(hback + 32 * n);
    const snapmi_error *b_errs = (const snapmi_error *)(hback + 40 * n);
    for (size_t i = 0; i < n; i++) {
        SeamReq *r = batch[i];
        r->err = b_errs[i];
        r->rc = b_errs[i].kind;
        r->written = b_errs[i].kind == SNAPMI_OK ? (size_t)b_out_lens[i] : 0;
        if (r->written > r->dev_out) { // cannot be: the device checks the caps
            r->rc = SNAPMI_E_DEVICE;
            r->written = 0;
        }
    }
}

struct SeamCombiner {
    std::deque<SeamReq *> q; // under g_pool.mu
    static constexpr size_t kMaxBatch = 1024;
    static constexpr size_t kMaxBytes = (size_t)1 << 30;
    // (under g_pool.mu) batches running now; when a request last had company
    size_t in_flight = 0;
    std::chrono::steady_clock::time_point last_company{};

    void run(SeamReq *r)
    {
        std::unique_lock<std::mutex> lock(g_pool.mu);
        r->state = 0;
        q.push_back(r);
        for (;;) {
            if (r->state == 2)
                return;
            if (r->state == 0) {
                bool none = false;
                snapmi_ctx *ctx = g_pool.checkout_locked(lock, false, &none);
                if (r->state != 0) { // (the lock was dropped meanwhile)
                    if (ctx) {
                        g_pool.idle.push_back(ctx);
                        g_pool.cv.notify_all();
                    }
                    continue;
                }
                if (none) { // no device: only this request fails here
                    for (auto it = q.begin(); it != q.end(); ++it)
                        if (*it == r) {
                            q.erase(it);
                            break;
                        }
                    r->rc = SNAPMI_E_DEVICE;
                    r->written = 0;
                    r->state = 2;
                    return;
                }
                if (ctx) {
                    lead(lock, ctx, r);
                    continue;
                }
            }
            g_pool.cv.wait(lock);
        }
    }
    // (mu held on entry and exit) gather, run, hand out
    void lead(std::unique_lock<std::mutex> &lock, snapmi_ctx *ctx, SeamReq *r)
    {
        // requests that are arriving right now join: until the queue has not
        // grown for ~8 us, 50 us at most (a call is ~1 500 us of GPU time) -
        // unless this caller has been alone for a while (no second request
        // queued or in flight during the last 2 ms): a single-threaded
        // caller pays no window at all
        const auto t_enter = std::chrono::steady_clock::now();
        if (q.size() > 1 || in_flight > 0)
            last_company = t_enter;
        if (t_enter - last_company <= std::chrono::milliseconds(2)) {
            size_t seen = q.size();
            lock.unlock();
            const auto t0 = std::chrono::steady_clock::now();
            auto t_grow = t0;
            for (;;) {
                std::this_thread::yield();
                const auto now = std::chrono::steady_clock::now();
                lock.lock();
                const size_t have = q.size();
                lock.unlock();
                if (have != seen) {
                    seen = have;
                    t_grow = now;
                }
                if (now - t_grow > std::chrono::microseconds(8) ||
                    now - t0 > std::chrono::microseconds(50))
                    break;
            }
            lock.lock();
        }
        if (r->state != 0) { // another leader took it during the window
            g_pool.idle.push_back(ctx);
            g_pool.cv.notify_all();
            return;
        }
        std::vector<SeamReq *> batch;
        size_t bytes = 0;
        for (auto it = q.begin(); it != q.end();) {
            SeamReq *x = *it;
            const size_t cost = x->in_len + x->dev_out;
            if (x->compress == r->compress &&
                (x == r || (batch.size() < kMaxBatch - 1 &&
                            bytes + cost <= kMaxBytes))) {
                x->state = 1;
                bytes += cost;
                batch.push_back(x);
                it = q.erase(it);
            } else {
                ++it;
            }
        }
        if (batch.size() > 1)
            last_company = std::chrono::steady_clock::now();
        in_flight++;
        lock.unlock();
        seam_execute(ctx, batch);
        lock.lock();
        in_flight--;
        for (SeamReq *x : batch)
            x->state = 2;
        g_pool.idle.push_back(ctx);
        g_pool.cv.notify_all();
    }
};
SeamCombiner g_seam;

// one seam call: through the combiner, or alone when the input is large
int seam_call(bool compress, const uint8_t *input, size_t input_len,
              uint8_t *output, size_t output_cap, size_t dev_out,
              size_t *written, const char *what)
{
    *written = 0;
    if (input_len > kPinStage || dev_out > kPinStage ||
        !tl_pin_in.reserve(input_len + 16) ||
        !tl_pin_out.reserve(dev_out + 64)) {
        SeamLease lease;
        snapmi_ctx *ctx = lease.ctx;
        if (!ctx) // (snapmi_ctx_create has printed why)
            return SNAPMI_E_DEVICE;
        snapmi_error err;
        const int rc = run_one(ctx, compress, input, input_len, output,
                               output_cap, written, &err);
        if (rc >= SNAPMI_E_DEVICE)
            fprintf(stderr, "snapmi: %s: %s\n", what, snapmi_last_error(ctx));
        return rc;
    }
    if (input_len)
        memcpy(tl_pin_in.p, input, input_len);
    SeamReq r;
    r.compress = compress;
    r.in_len = input_len;
    r.out_cap = output_cap;
    r.dev_out = dev_out;
    r.pin_in = (const uint8_t *)tl_pin_in.p;
    r.pin_out = (uint8_t *)tl_pin_out.p;
    r.rc = SNAPMI_E_DEVICE;
    r.written = 0;
    g_seam.run(&r);
    if (r.rc == SNAPMI_OK && r.written) {
        memcpy(output, r.pin_out, r.written);
        *written = r.written;
    }
    tl_pin_in.trim();
    tl_pin_out.trim();
    if (r.rc >= SNAPMI_E_DEVICE)
        fprintf(stderr, "snapmi: %s: device failure (no CPU fallback)\n",
                what);
    return r.rc;
}
} // namespace

size_t snappy_max_compressed_length(size_t source_length)
{
    return 32 + source_length + source_length / 6;
}

snappy_status snappy_uncompressed_length(const char *compressed,
                                         size_t compressed_length,
                                         size_t *result)
{
    // libsnappy reads a varint32: at most 5 bytes, value < 2^32.
    uint64_t v = 0;
    size_t n = compressed_length < 5 ? compressed_length : 5;
    size_t h = host_varint((const uint8_t *)compressed, n, &v);
    if (h == 0 || v > kMaxInput)
        return SNAPPY_INVALID_INPUT;
    *result = (size_t)v;
    return SNAPPY_OK;
}

snappy_status snappy_compress(const char *input, size_t input_length,
                              char *compressed, size_t *compressed_length)
{
    if (!compressed_length)
        return SNAPPY_INVALID_INPUT;
    if (*compressed_length < snappy_max_compressed_length(input_length))
        return SNAPPY_BUFFER_TOO_SMALL;
    size_t written = 0;
    size_t dev_out = snapmi_max_compress_len(input_length);
    if (dev_out == 0 || dev_out > *compressed_length)
        dev_out = *compressed_length;
    const int rc = seam_call(true, (const uint8_t *)input, input_length,
                             (uint8_t *)compressed, *compressed_length,
                             dev_out, &written, "snappy_compress");
    if (rc == SNAPMI_BUFFER_TOO_SMALL)
        return SNAPPY_BUFFER_TOO_SMALL;
    // (snappy_status has no "device" value: such a failure is printed and
    // reported as the one status a caller cannot mistake for success)
    if (rc != SNAPMI_OK)
        return SNAPPY_INVALID_INPUT;
    *compressed_length = written;
    return SNAPPY_OK;
}

snappy_status snappy_uncompress(const char *compressed,
                                size_t compressed_length, char *uncompressed,
                                size_t *uncompressed_length)
{
    if (!uncompressed_length)
        return SNAPPY_INVALID_INPUT;
    size_t need = 0;
    if (snappy_uncompressed_length(compressed, compressed_length, &need) !=
        SNAPPY_OK)
        return SNAPPY_INVALID_INPUT;
    if (*uncompressed_length < need)
        return SNAPPY_BUFFER_TOO_SMALL;
    size_t written = 0;
    const int rc = seam_call(false, (const uint8_t *)compressed,
                             compressed_length, (uint8_t *)uncompressed,
                             *uncompressed_length, need, &written,
                             "snappy_uncompress");
    if (rc != SNAPMI_OK)
        return SNAPPY_INVALID_INPUT;
    *uncompressed_length = written;
    return SNAPPY_OK;
}

snappy_status snappy_validate_compressed_buffer(const char *compressed,
                                                size_t compressed_length)
{
    size_t need = 0;
    if (snappy_uncompressed_length(compressed, compressed_length, &need) !=
        SNAPPY_OK)
        return SNAPPY_INVALID_INPUT;
    std::vector<char> tmp(need ? need : 1);
    size_t n = need;
    return snappy_uncompress(compressed, compressed_length, tmp.data(), &n);
}

} // extern "C"
