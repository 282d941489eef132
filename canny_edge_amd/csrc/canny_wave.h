// canny_wave.h -- the plain wave (64 lanes) and workgroup (256 threads) primitives of the feature kernels: butterfly sum /
// max / min, the inclusive prefix sum over a wave and the exclusive prefix sum over a workgroup.  Reductions that carry a
// payload (an arg-max pair, several sums at once, a carry across rounds) stay with their kernels.
//
// Device code only, everything forced inline and file-local.  A kernel file that had one of these as a function of its
// own compiles to the same instructions with the shared one.  That does not hold for a loop written out inside a kernel's
// own loop: the call unrolls before it is inlined and the surrounding code is scheduled differently, so such loops (the
// row scans of points, components, contours, edgels, ...) stay where they are unless the kernel is measured again.
// T is deduced from the argument: name it (wave_sum<unsigned long long>(n)) where the sum needs more bits than the value.
#ifndef CANNY_WAVE_H
#define CANNY_WAVE_H
#include <hip/hip_runtime.h>

namespace canny {

namespace {

// every lane receives the sum / the largest / the smallest of the wave's 64 values
template <typename T>
__device__ __forceinline__ T wave_sum(T v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

template <typename T>
__device__ __forceinline__ T wave_max(T v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const T t = __shfl_xor(v, d);
        v = t > v ? t : v;
    }
    return v;
}

template <typename T>
__device__ __forceinline__ T wave_min(T v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const T t = __shfl_xor(v, d);
        v = t < v ? t : v;
    }
    return v;
}

// lane i receives v of lanes 0 .. i; lane = threadIdx.x & 63
template <typename T>
__device__ __forceinline__ T wave_inclusive_scan(T v, int lane)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const T t = __shfl_up(v, d);
        if (lane >= d) v += t;
    }
    return v;
}

// Exclusive prefix of one value per thread over a 256-thread workgroup; *total receives the workgroup's sum.
// s_wave: 4 words of LDS, free for reuse after the call.
template <typename T>
__device__ __forceinline__ T block_exclusive_scan(T v, T *s_wave, T *total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const T incl = wave_inclusive_scan(v, lane);
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    T before = 0, sum = 0;
#pragma unroll
    for (int w = 0; w < 4; w++) {
        const T t = s_wave[w];
        if (w < wave) before += t;
        sum += t;
    }
    __syncthreads();
    *total = sum;
    return before + incl - v;
}

} // namespace

} // namespace canny

#endif
