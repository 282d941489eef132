// canny_descriptors.hip -- binary descriptors of the corners (256 intensity comparisons on the smoothed plane, optionally
// steered by the patch's intensity centroid) and brute-force Hamming matching between the descriptor sets of pairs of
// frames.  The rule is part of the interface (include/canny_hip.h); tests/descriptors_rule.py restates
// it in numpy and Python ints, canny_descriptors_host.cpp in plain C++.  All integers, no atomics, every output word has one
// writer: the same bytes on every run.
//
//   describe : one wave per corner slot, four waves a workgroup.  The wave stages the corner's 31 x 31 patch in LDS once,
//              with the clamped addresses (961 bytes, 16 byte loads a lane); the two moments come from the loaded registers by
//              a wave reduction, the 32 scores sit on the lanes and an arg-max on (score, smallest k) picks the rotation; lane
//              l then evaluates tests l, l + 64, l + 128, l + 192 from the rotated table (one dword a test) against the LDS
//              patch, and four ballots are the four words.
//   match    : one workgroup of 256 lanes per (pair, block of 256 queries); a lane keeps its query's four words in registers
//              and the train set streams through LDS in tiles of 1024 descriptors (32 KiB, every lane reads the same
//              address: a broadcast).  Per candidate XOR, popcount, add, and (d1, j1, d2) in registers.
//   reverse  : the same kernel with the roles swapped writes each train descriptor's best query into a workspace.
//   finalize : one workgroup per pair sets the flags and counts the accepted matches by a reduction.
#include "canny_kernels.h"

#include <algorithm>

namespace canny {

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kRadius = 15, kSide = 2 * kRadius + 1, kPatch = kSide * kSide; // 31, 961
constexpr int kPatchLds = 1024;                                              // 16 entries a lane
constexpr int kTile = 1024;                                                  // train descriptors of one LDS tile
constexpr int kNone = 257;                                                   // "no distance": above every distance
constexpr unsigned kGridCap = 2048;

// (ax, ay, bx, by) of test t in rotation k: the dword at (k * 256 + t)
__device__ const signed char __attribute__((aligned(4))) d_pattern[32 * 256 * 4] = {
#include "canny_desc_pattern.h"
};

// cos(2 pi k / 32) in Q14, k = 0..31; S_k = C_{(k - 8) & 31}
__device__ const int d_cos[32] = {16384,  16069,  15137,  13623,  11585,  9102,   6270,   3196,   0,      -3196, -6270,
                                  -9102,  -11585, -13623, -15137, -16069, -16384, -16069, -15137, -13623, -11585, -9102,
                                  -6270,  -3196,  0,      3196,   6270,   9102,   11585,  13623,  15137,  16069};

// grid plan_desc_slots; slots = n_frames * corners_max
template <class T>
__global__ __launch_bounds__(kBlock) void desc_describe_kernel(const T *__restrict__ plane, int h, int w,
                                                               const long long *__restrict__ corners,
                                                               const int *__restrict__ counts, int corners_max,
                                                               unsigned long long slots, int steered,
                                                               unsigned long long *__restrict__ desc, int *__restrict__ meta)
{
    __shared__ unsigned char s_patch[kWaves][kPatchLds];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    unsigned char *patch = s_patch[wave];
    // every wave of the workgroup takes the same number of trips: the barriers below are reached by all
    for (unsigned long long s0 = (unsigned long long)blockIdx.x * kWaves; s0 < slots; s0 += (unsigned long long)gridDim.x * kWaves) {
        const unsigned long long s = s0 + wave;
        bool live = s < slots, inside = false;
        int f = 0, cx = 0, cy = 0;
        if (live) {
            f = (int)(s / (unsigned)corners_max);
            live = (int)(s - (unsigned long long)f * (unsigned)corners_max) < counts[f];
        }
        if (live) {
            const long long x = corners[(size_t)s * 4], y = corners[(size_t)s * 4 + 1];
            inside = x >= 0 && x < w && y >= 0 && y < h;
            cx = (int)x, cy = (int)y;
            if (!inside) { // reads nothing: four zero words, meta -1
                if (lane < 4) desc[(size_t)s * 4 + lane] = 0;
                if (lane == 0) meta[s] = -1;
            }
        }
        int m10 = 0, m01 = 0;
        if (inside) {
            const T *img = plane + (size_t)f * h * w;
#pragma unroll
            for (int r = 0; r < kPatchLds / 64; r++) {
                const int i = lane + 64 * r;
                if (i < kPatch) {
                    const int py = i / kSide, px = i - py * kSide;
                    const int dy = py - kRadius, dx = px - kRadius;
                    const int yy = min(max(cy + dy, 0), h - 1), xx = min(max(cx + dx, 0), w - 1);
                    const int v = (int)img[(size_t)yy * w + xx] & 255;
                    patch[i] = (unsigned char)v;
                    if (dx * dx + dy * dy <= kRadius * kRadius) m10 += dx * v, m01 += dy * v;
                }
            }
        }
        __syncthreads();
        if (inside) {
            int k = 0;
            if (steered) {
                for (int d = 32; d > 0; d >>= 1) {
                    m10 += __shfl_xor(m10, d);
                    m01 += __shfl_xor(m01, d);
                }
                k = lane & 31; // lanes l and l + 32 hold the same candidate
                long long score = (long long)m10 * d_cos[k] + (long long)m01 * d_cos[(k - 8) & 31];
                for (int d = 16; d > 0; d >>= 1) {
                    const long long s2 = __shfl_xor(score, d);
                    const int k2 = __shfl_xor(k, d);
                    if (s2 > score || (s2 == score && k2 < k)) score = s2, k = k2;
                }
            }
            const int *table = (const int *)d_pattern + k * 256;
            unsigned long long word[4];
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const int t = table[lane + 64 * q];
                const int ax = (signed char)t, ay = (signed char)(t >> 8), bx = (signed char)(t >> 16), by = t >> 24;
                const int a = patch[(kRadius + ay) * kSide + kRadius + ax], b = patch[(kRadius + by) * kSide + kRadius + bx];
                word[q] = __ballot(a < b);
            }
            const unsigned long long mine = lane == 0 ? word[0] : lane == 1 ? word[1] : lane == 2 ? word[2] : word[3];
            if (lane < 4) desc[(size_t)s * 4 + lane] = mine;
            if (lane == 0) {
                const int border = cx - kRadius < 0 || cy - kRadius < 0 || cx + kRadius > w - 1 || cy + kRadius > h - 1;
                meta[s] = k + 256 * border;
            }
        }
        __syncthreads(); // the patch has been read
    }
}

// grid plan_desc_match; units = n_pairs * blocks, blocks = ceil(stride_q / 256).  "q" is the side whose descriptors sit in
// registers; with REVERSE the caller passes the train set as q and the query set as t, and pairs are read the other way
// round.  Forward: out is [n_pairs][stride_q][4] ints and receives j, d1, d2; reverse: out is [n_pairs][stride_q] ints, j only.
template <bool REVERSE>
__global__ __launch_bounds__(kBlock) void desc_match_kernel(const unsigned long long *__restrict__ q_desc,
                                                            const int *__restrict__ q_counts, int stride_q,
                                                            const unsigned long long *__restrict__ t_desc,
                                                            const int *__restrict__ t_counts, int stride_t,
                                                            const int *__restrict__ pairs, unsigned units, unsigned blocks,
                                                            int *__restrict__ out)
{
    __shared__ __attribute__((aligned(16))) unsigned long long s_tile[kTile * 4];
    const int tid = threadIdx.x;
    for (unsigned u = blockIdx.x; u < units; u += gridDim.x) {
        const unsigned p = u / blocks, b = u - p * blocks;
        const int fq = pairs[2 * p + (REVERSE ? 1 : 0)], ft = pairs[2 * p + (REVERSE ? 0 : 1)];
        const int nq = min(max(q_counts[fq], 0), stride_q), nt = min(max(t_counts[ft], 0), stride_t);
        if ((int)(b * kBlock) >= nq) continue; // the same for the whole workgroup
        const int i = (int)(b * kBlock) + tid;
        unsigned long long w0 = 0, w1 = 0, w2 = 0, w3 = 0;
        if (i < nq) {
            const unsigned long long *q = q_desc + ((size_t)fq * stride_q + i) * 4;
            w0 = q[0], w1 = q[1], w2 = q[2], w3 = q[3];
        }
        int d1 = kNone, d2 = kNone, j1 = -1;
        const unsigned long long *train = t_desc + (size_t)ft * stride_t * 4;
        for (int t0 = 0; t0 < nt; t0 += kTile) {
            const int tn = min(kTile, nt - t0);
            __syncthreads(); // the previous tile has been read
            for (int e = tid; e < tn * 4; e += kBlock) s_tile[e] = train[(size_t)t0 * 4 + e];
            __syncthreads();
            const ulonglong2 *tile = (const ulonglong2 *)s_tile;
#pragma unroll 4 // four candidates' LDS reads in flight before the first popcount waits
            for (int c = 0; c < tn; c++) {
                const ulonglong2 lo = tile[2 * c], hi = tile[2 * c + 1];
                const int d = __popcll(lo.x ^ w0) + __popcll(lo.y ^ w1) + __popcll(hi.x ^ w2) + __popcll(hi.y ^ w3);
                // j ascends, so a strict < keeps the smallest j of the smallest distance
                if (d < d1) d2 = d1, d1 = d, j1 = t0 + c;
                else if (d < d2) d2 = d;
            }
        }
        if (i < nq) {
            if (REVERSE) {
                out[(size_t)p * stride_q + i] = j1;
            } else {
                int *m = out + ((size_t)p * stride_q + i) * 4;
                m[0] = j1, m[1] = d1, m[2] = d2;
            }
        }
    }
}

// grid n_pairs.  back: [n_pairs][stride_t] ints, per train descriptor its best query.
__global__ __launch_bounds__(kBlock) void desc_finalize_kernel(const int *__restrict__ q_counts, int stride_q, int stride_t,
                                                               const int *__restrict__ pairs, const int *__restrict__ back,
                                                               int max_distance, int ratio_q8, int cross,
                                                               int *__restrict__ matches, int *__restrict__ pair_counts)
{
    __shared__ int s_wave[kWaves];
    const unsigned p = blockIdx.x;
    const int tid = threadIdx.x;
    const int nq = min(max(q_counts[pairs[2 * p]], 0), stride_q);
    int n_acc = 0;
    for (int i = tid; i < nq; i += kBlock) {
        int *m = matches + ((size_t)p * stride_q + i) * 4;
        const int j = m[0], d1 = m[1], d2 = m[2];
        const int f0 = d1 <= max_distance, f1 = ratio_q8 == 0 || d1 * 256 < ratio_q8 * d2;
        const int mutual = j >= 0 && back[(size_t)p * stride_t + j] == i;
        const int acc = f0 && f1 && (mutual || !cross);
        m[3] = f0 | f1 << 1 | mutual << 2 | acc << 3;
        n_acc += acc;
    }
    for (int d = 32; d > 0; d >>= 1) n_acc += __shfl_xor(n_acc, d);
    if ((tid & 63) == 0) s_wave[tid >> 6] = n_acc;
    __syncthreads();
    if (tid == 0) pair_counts[p] = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
}

} // namespace

LaunchPlan plan_desc_slots(unsigned long long slots) { return capped_plan(slots, kWaves, kGridCap); }
LaunchPlan plan_desc_match(unsigned long long n_pairs, int stride)
{
    return capped_plan(n_pairs * (unsigned long long)((stride + kBlock - 1) / kBlock), 1, kGridCap);
}

hipError_t launch_desc_describe(const void *plane, bool plane_u8, int n_frames, int height, int width,
                                const long long *corners, const int *counts, int corners_max, int steered,
                                unsigned long long *desc, int *meta, hipStream_t stream)
{
    if (n_frames < 1 || corners_max < 1 || corners_max > kHoughMaxLines || height < 2 || width < 2)
        return hipErrorInvalidValue;
    const unsigned long long slots = (unsigned long long)n_frames * corners_max;
    const LaunchPlan p = plan_desc_slots(slots);
    if (plane_u8)
        hipLaunchKernelGGL(desc_describe_kernel<uint8_t>, dim3(p.grid), dim3(kBlock), 0, stream, (const uint8_t *)plane,
                           height, width, corners, counts, corners_max, slots, steered, desc, meta);
    else
        hipLaunchKernelGGL(desc_describe_kernel<int16_t>, dim3(p.grid), dim3(kBlock), 0, stream, (const int16_t *)plane,
                           height, width, corners, counts, corners_max, slots, steered, desc, meta);
    return hipGetLastError();
}

hipError_t launch_desc_match(const unsigned long long *q_desc, const int *q_counts, int stride_q,
                             const unsigned long long *t_desc, const int *t_counts, int stride_t, const int *pairs,
                             int n_pairs, bool reverse, int *out, hipStream_t stream)
{
    if (n_pairs < 1 || stride_q < 1 || stride_t < 1 || stride_q > kHoughMaxLines || stride_t > kHoughMaxLines)
        return hipErrorInvalidValue;
    const LaunchPlan p = plan_desc_match((unsigned long long)n_pairs, stride_q);
    const unsigned blocks = (unsigned)((stride_q + kBlock - 1) / kBlock);
    if (reverse)
        hipLaunchKernelGGL(desc_match_kernel<true>, dim3(p.grid), dim3(kBlock), 0, stream, q_desc, q_counts, stride_q,
                           t_desc, t_counts, stride_t, pairs, (unsigned)p.units, blocks, out);
    else
        hipLaunchKernelGGL(desc_match_kernel<false>, dim3(p.grid), dim3(kBlock), 0, stream, q_desc, q_counts, stride_q,
                           t_desc, t_counts, stride_t, pairs, (unsigned)p.units, blocks, out);
    return hipGetLastError();
}

hipError_t launch_desc_finalize(const int *q_counts, int stride_q, int stride_t, const int *pairs, int n_pairs,
                                const int *back, int max_distance, int ratio_q8, int cross, int *matches, int *pair_counts,
                                hipStream_t stream)
{
    if (n_pairs < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(desc_finalize_kernel, dim3(n_pairs), dim3(kBlock), 0, stream, q_counts, stride_q, stride_t, pairs,
                       back, max_distance, ratio_q8, cross, matches, pair_counts);
    return hipGetLastError();
}

} // namespace canny
