// canny_to_gray.hip -- interleaved colour frames (BGR / RGB / BGRA / RGBA, 8 bits per channel) -> the 1-byte gray plane
// every other stage takes: the reference's caller does this with cv::cvtColor before canny() (src/main.cpp:114).
//
// The standalone pass (the fused form lives in the marching Gaussian, canny_gaussian_march.hip): the batch is one flat
// array of n_px pixels.  Each lane converts 16 pixels -- 16*CH source bytes in 3 or 4 dwordx4 loads, one
// dwordx4 store -- through gray4(), the arithmetic the fused kernel uses too.  The source may sit at any byte address
// (a frame inside a caller's buffer): the loads are unaligned dword loads, which gfx950 serves at full width.  The last
// n_px % 16 pixels are done in 4-pixel groups by the first lanes of block 0, byte by byte.
// HBM traffic: CH bytes in + 1 byte out per pixel.
#include "canny_kernels.h"

namespace canny {

namespace {

template <int CH>
__global__ __launch_bounds__(256) void to_gray_kernel(const uint8_t *__restrict__ src, uint8_t *__restrict__ gray,
                                                      size_t n_px, GrayRule rule)
{
    const size_t n_groups = n_px / 16;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x; g < n_groups; g += stride) {
        uint32_t w[4 * CH];
        __builtin_memcpy(w, src + g * 16 * CH, 16 * CH);
        uint32_t o[4];
#pragma unroll
        for (int q = 0; q < 4; q++) o[q] = gray4<CH>(w + q * CH, rule);
        __builtin_memcpy(gray + g * 16, o, 16);
    }
    // tail: up to 15 pixels, as up to four groups of four (missing pixels read as zeros and are not stored)
    const size_t tail0 = n_groups * 16;
    if (blockIdx.x == 0 && tail0 + 4 * threadIdx.x < n_px) {
        const size_t p0 = tail0 + 4 * threadIdx.x;
        const int np = (int)min<size_t>(4, n_px - p0);
        uint32_t w[CH] = {};
        for (int b = 0; b < np * CH; b++) w[b >> 2] |= (uint32_t)src[p0 * CH + b] << (8 * (b & 3));
        const uint32_t o = gray4<CH>(w, rule);
        for (int p = 0; p < np; p++) gray[p0 + p] = (uint8_t)(o >> (8 * p));
    }
}

} // namespace

// enough waves to fill the chip several times over; the grid-stride loop takes the rest
LaunchPlan plan_to_gray(size_t n_px) { return capped_plan(n_px / 16, 256, 8192); }

hipError_t launch_to_gray(const uint8_t *src, int ch, const GrayRule &rule, uint8_t *gray, size_t n_px,
                          hipStream_t stream)
{
    if (n_px == 0) return hipSuccess;
    const unsigned blocks = plan_to_gray(n_px).grid;
    if (ch == 3)
        hipLaunchKernelGGL(to_gray_kernel<3>, dim3(blocks), dim3(256), 0, stream, src, gray, n_px, rule);
    else if (ch == 4)
        hipLaunchKernelGGL(to_gray_kernel<4>, dim3(blocks), dim3(256), 0, stream, src, gray, n_px, rule);
    else
        return hipErrorInvalidValue;
    return hipGetLastError();
}

} // namespace canny
