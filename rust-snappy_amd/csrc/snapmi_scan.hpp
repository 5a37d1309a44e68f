// snapmi_scan.hpp -- the exclusive prefix sum of a workgroup, once (device).
//
// Every batch call turns counts into offsets with it: the planner's blocks
// and slots, the blocks' output offsets, the block index's first[], the frame
// codec's chunk offsets, the pieces and rooms of a group of ranges, the
// touched blocks' growth and the splice jobs of a group of writes.  The sites
// differ only in what they load and what they store: they pass that as two
// callables and keep their own rules (clamps, carries from a segment in
// front, rejections, who writes a total) around the call.
//
// T is uint32_t or uint64_t, N (1 or 2) the number of values scanned
// together: item i's values are T x[N], the scans of x[0] and x[1] run side
// by side.  The loops over N have constant bounds and unroll.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace snapmi {

// The workgroup scan.  ex[k] = the sum of x[k] over the threads in front of
// this one, total[k] = the sum over the whole workgroup (in every thread).
// Contract: EVERY thread of the workgroup calls it (no divergent call, no
// early return in front of it that is not workgroup-uniform); blockDim.x is a
// multiple of 64 and at most 1024.  Inside the wave 6 __shfl_up steps, then
// the waves' totals through 16 x N words of LDS; it ends with the barrier
// that frees those words for the next call.
template <class T, int N>
__device__ __forceinline__ void wg_scan(const T (&x)[N], T (&ex)[N],
                                        T (&total)[N])
{
    __shared__ T wave_tot[16][N];
    const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    T s[N]; // inclusive inside the wave
    for (int k = 0; k < N; k++)
        s[k] = x[k];
    for (uint32_t o = 1; o < 64; o <<= 1) {
        T t[N];
        for (int k = 0; k < N; k++)
            t[k] = __shfl_up(s[k], o);
        if (lane >= o)
            for (int k = 0; k < N; k++)
                s[k] += t[k];
    }
    if (lane == 63)
        for (int k = 0; k < N; k++)
            wave_tot[w][k] = s[k];
    __syncthreads();
    T before[N];
    for (int k = 0; k < N; k++)
        before[k] = total[k] = 0;
    for (uint32_t j = 0; j < (blockDim.x >> 6); j++)
        for (int k = 0; k < N; k++) {
            const T t = wave_tot[j][k];
            if (j < w)
                before[k] += t;
            total[k] += t;
        }
    __syncthreads();
    for (int k = 0; k < N; k++)
        ex[k] = before[k] + s[k] - x[k];
}

// The strided scan of items [0, n) on ONE workgroup, blockDim.x items a
// stride: load(i, x) fills item i's values, store(i, x, ex) takes them back
// with the item's exclusive sum, carry included.  carry goes in as the sum in
// front of item 0 and comes out with the total added, in every thread.  Same
// contract as wg_scan; n is workgroup-uniform.
template <class T, int N, class Load, class Store>
__device__ __forceinline__ void wg_scan_strided(uint32_t n, T (&carry)[N],
                                                Load load, Store store)
{
    for (uint32_t base = 0; base < n; base += blockDim.x) {
        const uint32_t i = base + threadIdx.x;
        T x[N] = {}, ex[N], total[N];
        if (i < n)
            load(i, x);
        wg_scan(x, ex, total);
        for (int k = 0; k < N; k++)
            ex[k] += carry[k];
        if (i < n)
            store(i, x, ex);
        for (int k = 0; k < N; k++)
            carry[k] += total[k];
    }
}

// The scan of n items on many workgroups of blockDim.x items each, three
// launches; part holds N words per workgroup.
// (a) every workgroup scans its items - store gets the exclusive sum within
//     the workgroup - and leaves its totals in part;
template <class T, int N, class Load, class Store>
__device__ __forceinline__ void wg_scan_a(uint32_t n, T *part, Load load,
                                          Store store)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    T x[N] = {}, ex[N], total[N];
    if (i < n)
        load(i, x);
    wg_scan(x, ex, total);
    if (i < n)
        store(i, x, ex);
    if (threadIdx.x == 0)
        for (int k = 0; k < N; k++)
            part[N * blockIdx.x + k] = total[k];
}

// (b) one workgroup turns the nparts totals into offsets, in place (carry as
//     for wg_scan_strided: the site writes the total where it wants one);
template <class T, int N>
__device__ __forceinline__ void wg_scan_b(T *part, uint32_t nparts,
                                          T (&carry)[N])
{
    wg_scan_strided(
        nparts, carry,
        [&](uint32_t j, T (&x)[N]) {
            for (int k = 0; k < N; k++)
                x[k] = part[N * j + k];
        },
        [&](uint32_t j, const T (&)[N], const T (&ex)[N]) {
            for (int k = 0; k < N; k++)
                part[N * j + k] = ex[k];
        });
}

// (c) every workgroup adds its offset: add(i, off) for item i < n.
template <class T, int N, class Add>
__device__ __forceinline__ void wg_scan_c(uint32_t n, const T *part, Add add)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n)
        return;
    T off[N];
    for (int k = 0; k < N; k++)
        off[k] = part[N * blockIdx.x + k];
    add(i, off);
}

} // namespace snapmi
