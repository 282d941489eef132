// canny_motion.hip -- frame-to-frame motion from the corner matches: consensus (RANSAC) over the accepted matches of a pair of
// frames and one motion model (translation, similarity, affine) fitted to the ones that agree.  The rule is part of the
// interface (include/canny_hip.h); tests/motion_rule.py restates it in numpy and Python ints,
// canny_motion_host.cpp in plain C++.  All integers, no atomics, every output word has one writer: the same bytes on every run.
//
//   gather : one workgroup per pair walks the query slots 256 at a time; ballots and prefix sums compact the
//            correspondences in query order: (x, y, x', y') as four u16 in one word and the slot index go to the workspace, m too, and
//            the slots that are no correspondence get their -1 flag.
//   score  : one workgroup of 256 lanes per (pair, block of 256 hypotheses).  The pair's list is staged in LDS (8 B a
//            correspondence, 32 KiB at most), a lane builds its hypothesis in registers (D, M, the first sample, the
//            threshold floor(thr^2 D^2 / 256) in 128 bits) and the list streams by with every lane reading the same LDS
//            address: a broadcast.  Per test two 64-bit residuals and two 64 x 64 -> 128 squares.  One int per (pair, h).
//   refit  : one workgroup per pair: arg-max over (count desc, h asc), the inlier pass with the flags and the eleven sums
//            (wave reductions), the 128-bit algebra with a restoring division on one lane, the residual pass, the record.
#include "canny_kernels.h"
#include "canny_wave.h"

namespace canny {

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kListMax = kHoughMaxLines; // correspondences of a pair: 32 KiB of LDS
constexpr unsigned kGridCap = 2048;
constexpr long long kLimit = 1ll << 24;  // largest |a_ij| of a refit, Q16
constexpr int kWords = 16;               // CANNY_HIP_MOTION_WORDS
constexpr int kMaxHypotheses = 4096;     // CANNY_HIP_MOTION_MAX_HYPOTHESES

typedef __int128 i128;
typedef unsigned __int128 u128;

// a correspondence as the workspace holds it: x | y << 16 | x' << 32 | y' << 48
typedef unsigned long long Packed;
struct Corr {
    int x, y, u, v; // query (x, y) -> train (u, v)
};
__device__ __forceinline__ Corr mt_unpack(Packed v)
{
    return Corr{(int)(v & 0xffff), (int)((v >> 16) & 0xffff), (int)((v >> 32) & 0xffff), (int)(v >> 48)};
}

struct Hyp {
    long long D, m11, m12, m21, m22;
    int x1, y1, u1, v1;
    unsigned long long lim_hi, lim_lo; // floor(thr^2 D^2 / 256): X <= limit iff 256 X <= thr^2 D^2
};

__device__ __forceinline__ unsigned mt_draw(unsigned &s, unsigned n)
{
    s = s * 1664525u + 1013904223u;
    return (s >> 16) % n;
}

// the first `model + 1` sample indices of hypothesis h among m >= model + 1 correspondences; the others are 0
__device__ __forceinline__ void mt_sample(unsigned seed, int h, int m, int model, int &i1, int &i2, int &i3)
{
    unsigned s = seed + 0x9E3779B9u * (unsigned)(h + 1);
    i1 = (int)mt_draw(s, (unsigned)m), i2 = 0, i3 = 0;
    if (model >= 1) {
        i2 = (int)mt_draw(s, (unsigned)(m - 1));
        i2 += i2 >= i1;
    }
    if (model >= 2) {
        i3 = (int)mt_draw(s, (unsigned)(m - 2));
        i3 += i3 >= min(i1, i2);
        i3 += i3 >= max(i1, i2);
    }
}

// false: D == 0.  |D| <= 2^33, |M| <= 2^34: every product below is of two values under 2^17.
__device__ __forceinline__ bool mt_build(int model, Corr a, Corr b, Corr f, int thr_q4, Hyp &o)
{
    o.x1 = a.x, o.y1 = a.y, o.u1 = a.u, o.v1 = a.v;
    if (model == 0) {
        o.D = 1, o.m11 = o.m22 = 1, o.m12 = o.m21 = 0;
    } else {
        const long long dx = b.x - a.x, dy = b.y - a.y, du = b.u - a.u, dv = b.v - a.v;
        if (model == 1) {
            const long long A = dx * du + dy * dv, B = dx * dv - dy * du;
            o.D = dx * dx + dy * dy;
            o.m11 = A, o.m12 = -B, o.m21 = B, o.m22 = A;
        } else {
            const long long fx = f.x - a.x, fy = f.y - a.y, fu = f.u - a.u, fv = f.v - a.v;
            o.D = dx * fy - dy * fx;
            o.m11 = du * fy - fu * dy, o.m12 = fu * dx - du * fx;
            o.m21 = dv * fy - fv * dy, o.m22 = fv * dx - dv * fx;
        }
    }
    const unsigned long long aD = (unsigned long long)(o.D < 0 ? -o.D : o.D);
    // thr^2 < 2^24, D^2 <= 2^66: under 2^90
    const u128 limit = (((u128)aD * aD) * (unsigned long long)((unsigned)thr_q4 * (unsigned)thr_q4)) >> 8;
    o.lim_hi = (unsigned long long)(limit >> 64), o.lim_lo = (unsigned long long)limit;
    return o.D != 0;
}

// r = D (c' - q1') - M (c - q1), |r| < 2^53; rx^2 + ry^2 < 2^107
__device__ __forceinline__ bool mt_inlier(const Hyp &h, Corr c)
{
    const long long dx = c.x - h.x1, dy = c.y - h.y1, du = c.u - h.u1, dv = c.v - h.v1;
    const long long rx = h.D * du - (h.m11 * dx + h.m12 * dy), ry = h.D * dv - (h.m21 * dx + h.m22 * dy);
    const unsigned long long ax = (unsigned long long)(rx < 0 ? -rx : rx), ay = (unsigned long long)(ry < 0 ? -ry : ry);
    return (u128)ax * ax + (u128)ay * ay <= (((u128)h.lim_hi << 64) | h.lim_lo);
}

// floor(n / d), d > 0: restoring division, one bit a step (there is no 128-bit division on the device)
__device__ i128 mt_floor_div(i128 n, i128 d)
{
    u128 a = n < 0 ? (u128)0 - (u128)n : (u128)n, q = 0, r = 0;
    const u128 ud = (u128)d;
    for (int i = 0; i < 128; i++) {
        r = (r << 1) | (a >> 127);
        a <<= 1;
        q <<= 1;
        if (r >= ud) r -= ud, q |= 1;
    }
    i128 s = (i128)q;
    if (n < 0) s = -s - (r != 0 ? 1 : 0);
    return s;
}

__device__ __forceinline__ long long mt_floor_div64(long long n, long long d) // d > 0
{
    long long q = n / d;
    if (n % d != 0 && n < 0) q--;
    return q;
}

// grid plan_motion_pairs.  list, slot: [n_pairs][stride_q]; m_out: [n_pairs]
__global__ __launch_bounds__(kBlock) void motion_gather_kernel(const long long *__restrict__ q_corners,
                                                               const int *__restrict__ q_counts, int stride_q,
                                                               const long long *__restrict__ t_corners,
                                                               const int *__restrict__ t_counts, int stride_t,
                                                               const int *__restrict__ pairs, unsigned n_pairs,
                                                               const int *__restrict__ matches, Packed *__restrict__ list,
                                                               int *__restrict__ slot, int *__restrict__ m_out,
                                                               int *__restrict__ inlier)
{
    __shared__ int s_wave[kWaves];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    for (unsigned p = blockIdx.x; p < n_pairs; p += gridDim.x) {
        const int fq = pairs[2 * p], ft = pairs[2 * p + 1];
        const int nq = min(max(q_counts[fq], 0), stride_q), nt = min(max(t_counts[ft], 0), stride_t);
        const size_t row = (size_t)p * stride_q;
        int base = 0; // the same on every lane
        for (int i0 = 0; i0 < nq; i0 += kBlock) {
            const int i = i0 + tid;
            bool is = false;
            Packed c = 0;
            if (i < nq) {
                const int *mt = matches + (row + i) * 4;
                const int j = mt[0], flags = mt[3];
                if ((flags & 8) && j >= 0 && j < nt) {
                    const long long *q = q_corners + ((size_t)fq * stride_q + i) * 4;
                    const long long *t = t_corners + ((size_t)ft * stride_t + j) * 4;
                    const long long x = q[0], y = q[1], u = t[0], v = t[1];
                    is = x >= 0 && x <= 65535 && y >= 0 && y <= 65535 && u >= 0 && u <= 65535 && v >= 0 && v <= 65535;
                    c = (Packed)x | (Packed)y << 16 | (Packed)u << 32 | (Packed)v << 48; // only kept if all four fit
                }
                if (inlier && !is) inlier[row + i] = -1;
            }
            const unsigned long long ballot = __ballot(is);
            const int before = __popcll(ballot & ((1ull << lane) - 1));
            if (lane == 0) s_wave[wave] = __popcll(ballot);
            __syncthreads();
            int at = base + before, total = 0;
#pragma unroll
            for (int w = 0; w < kWaves; w++) {
                const int n = s_wave[w];
                if (w < wave) at += n;
                total += n;
            }
            if (is) { // at < nq <= stride_q: at most one correspondence a slot
                list[row + at] = c;
                slot[row + at] = i;
            }
            base += total;
            __syncthreads(); // the wave counts have been read
        }
        if (tid == 0) m_out[p] = base;
    }
}

// grid plan_motion_score; units = n_pairs * blocks, blocks = ceil(hypotheses / 256).  counts: [n_pairs][hypotheses], -1 for
// a hypothesis that is invalid
__global__ __launch_bounds__(kBlock) void motion_score_kernel(const Packed *__restrict__ list, const int *__restrict__ m_in,
                                                              int stride_q, unsigned units, unsigned blocks, int model,
                                                              int thr_q4, int hypotheses, unsigned seed,
                                                              int *__restrict__ counts)
{
    __shared__ Packed s_list[kListMax];
    const int tid = threadIdx.x;
    for (unsigned u = blockIdx.x; u < units; u += gridDim.x) {
        const unsigned p = u / blocks, b = u - p * blocks;
        const int m = min(m_in[p], min(stride_q, kListMax)); // m <= stride_q by construction: the bound the LDS list needs
        const int h = (int)(b * kBlock) + tid;
        int count = -1;
        if (m > model) { // the same for the whole workgroup
            __syncthreads(); // the previous list has been read
            const Packed *src = list + (size_t)p * stride_q;
            for (int e = tid; e < m; e += kBlock) s_list[e] = src[e];
            __syncthreads();
            int i1, i2, i3;
            mt_sample(seed, h, m, model, i1, i2, i3);
            Hyp hy;
            const bool valid = mt_build(model, mt_unpack(s_list[i1]), mt_unpack(s_list[i2]), mt_unpack(s_list[i3]), thr_q4, hy);
            int n = 0;
#pragma unroll 4 // four broadcast reads in flight before the first product waits
            for (int e = 0; e < m; e++) n += mt_inlier(hy, mt_unpack(s_list[e])) ? 1 : 0;
            if (valid) count = n;
        }
        if (h < hypotheses) counts[(size_t)p * hypotheses + h] = count;
    }
}

// grid plan_motion_pairs
__global__ __launch_bounds__(kBlock) void motion_refit_kernel(const Packed *__restrict__ list, const int *__restrict__ slot,
                                                              const int *__restrict__ m_in, int stride_q, unsigned n_pairs,
                                                              const int *__restrict__ counts, int model, int thr_q4,
                                                              int hypotheses, unsigned seed, long long *__restrict__ motion,
                                                              int *__restrict__ inlier)
{
    constexpr int kSums = 12;
    __shared__ long long s_sum[kWaves][kSums];
    __shared__ long long s_fit[8];
    __shared__ int s_best[kWaves][2];
    __shared__ unsigned char s_in[kListMax];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    for (unsigned p = blockIdx.x; p < n_pairs; p += gridDim.x) {
        __syncthreads(); // the previous pair's shared words have been read
        const int m = min(m_in[p], min(stride_q, kListMax));
        const size_t row = (size_t)p * stride_q;
        const Packed *lp = list + row;
        long long *rec = motion + (size_t)p * kWords;
        // the best hypothesis: most inliers, then the smallest h
        int bn = -1, bh = 0x7fffffff;
        for (int h = tid; h < hypotheses; h += kBlock) {
            const int n = counts[(size_t)p * hypotheses + h];
            if (n > bn) bn = n, bh = h;
        }
        for (int d = 32; d > 0; d >>= 1) {
            const int n2 = __shfl_xor(bn, d), h2 = __shfl_xor(bh, d);
            if (n2 > bn || (n2 == bn && h2 < bh)) bn = n2, bh = h2;
        }
        if (lane == 0) s_best[wave][0] = bn, s_best[wave][1] = bh;
        __syncthreads();
        bn = s_best[0][0], bh = s_best[0][1];
#pragma unroll
        for (int w = 1; w < kWaves; w++) {
            const int n2 = s_best[w][0], h2 = s_best[w][1];
            if (n2 > bn || (n2 == bn && h2 < bh)) bn = n2, bh = h2;
        }
        if (bn < 0) { // no model: the same for the whole workgroup
            if (inlier)
                for (int e = tid; e < m; e += kBlock) inlier[row + slot[row + e]] = 0;
            if (tid < kWords) rec[tid] = tid == 1 ? m : (tid == 3 || (tid >= 12 && tid <= 14)) ? -1 : 0;
            continue;
        }
        int i1, i2, i3;
        mt_sample(seed, bh, m, model, i1, i2, i3);
        Hyp hy;
        mt_build(model, mt_unpack(lp[i1]), mt_unpack(lp[i2]), mt_unpack(lp[i3]), thr_q4, hy);
        long long s[kSums];
#pragma unroll
        for (int k = 0; k < kSums; k++) s[k] = 0;
        for (int e = tid; e < m; e += kBlock) {
            const Corr c = mt_unpack(lp[e]);
            const bool in = mt_inlier(hy, c);
            s_in[e] = in; // read back by this lane only
            if (inlier) inlier[row + slot[row + e]] = in ? 1 : 0;
            if (in) {
                const long long x = c.x, y = c.y, u = c.u, v = c.v;
                s[0] += 1, s[1] += x, s[2] += y, s[3] += u, s[4] += v;
                s[5] += x * x, s[6] += x * y, s[7] += y * y, s[8] += x * u, s[9] += x * v, s[10] += y * u, s[11] += y * v;
            }
        }
#pragma unroll
        for (int k = 0; k < kSums; k++) {
            const long long v = wave_sum(s[k]);
            if (lane == 0) s_sum[wave][k] = v;
        }
        __syncthreads();
        if (tid == 0) {
#pragma unroll
            for (int k = 0; k < kSums; k++) s[k] = s_sum[0][k] + s_sum[1][k] + s_sum[2][k] + s_sum[3][k];
            const long long n = s[0], sx = s[1], sy = s[2], su = s[3], sv = s[4];
            // |C| <= n^2 2^30 <= 2^54; the two terms of each stay under 2^57
            const long long cxx = n * s[5] - sx * sx, cxy = n * s[6] - sx * sy, cyy = n * s[7] - sy * sy;
            const long long cxu = n * s[8] - sx * su, cxv = n * s[9] - sx * sv, cyu = n * s[10] - sy * su, cyv = n * s[11] - sy * sv;
            i128 a11 = 65536, a12 = 0, a21 = 0, a22 = 65536;
            bool ok = true;
            if (model == 1) {
                const i128 dn = (i128)cxx + cyy;
                ok = dn > 0;
                if (ok) {
                    a11 = a22 = mt_floor_div(((i128)cxu + cyv) * 65536, dn);
                    a21 = mt_floor_div(((i128)cxv - cyu) * 65536, dn);
                    a12 = -a21;
                }
            } else if (model == 2) {
                const i128 det = (i128)cxx * cyy - (i128)cxy * cxy;
                ok = det > 0;
                if (ok) { // numerators under 2^110, times 65536 under 2^126
                    a11 = mt_floor_div(((i128)cxu * cyy - (i128)cyu * cxy) * 65536, det);
                    a12 = mt_floor_div(((i128)cyu * cxx - (i128)cxu * cxy) * 65536, det);
                    a21 = mt_floor_div(((i128)cxv * cyy - (i128)cyv * cxy) * 65536, det);
                    a22 = mt_floor_div(((i128)cyv * cxx - (i128)cxv * cxy) * 65536, det);
                }
            }
            ok = ok && a11 <= kLimit && a11 >= -kLimit && a12 <= kLimit && a12 >= -kLimit && a21 <= kLimit &&
                 a21 >= -kLimit && a22 <= kLimit && a22 >= -kLimit;
            long long tx = 0, ty = 0;
            if (ok) {
                tx = mt_floor_div64(65536 * su - (long long)a11 * sx - (long long)a12 * sy, n);
                ty = mt_floor_div64(65536 * sv - (long long)a21 * sx - (long long)a22 * sy, n);
            }
            s_fit[0] = ok ? (long long)a11 : 0, s_fit[1] = ok ? (long long)a12 : 0, s_fit[2] = tx;
            s_fit[3] = ok ? (long long)a21 : 0, s_fit[4] = ok ? (long long)a22 : 0, s_fit[5] = ty;
            s_fit[6] = ok, s_fit[7] = n;
        }
        __syncthreads();
        const bool ok = s_fit[6] != 0;
        long long total = 0, worst = 0;
        if (ok) {
            const long long a11 = s_fit[0], a12 = s_fit[1], tx = s_fit[2], a21 = s_fit[3], a22 = s_fit[4], ty = s_fit[5];
            for (int e = tid; e < m; e += kBlock) {
                if (!s_in[e]) continue;
                const Corr c = mt_unpack(lp[e]);
                long long gx = (65536ll * c.u - (a11 * c.x + a12 * c.y + tx)) >> 8;
                long long gy = (65536ll * c.v - (a21 * c.x + a22 * c.y + ty)) >> 8;
                gx = min(max(gx, -kLimit), kLimit), gy = min(max(gy, -kLimit), kLimit);
                const long long g = gx * gx + gy * gy;
                total += g;
                worst = max(worst, g);
            }
        }
        total = wave_sum(total);
        for (int d = 32; d > 0; d >>= 1) worst = max(worst, __shfl_xor(worst, d));
        __syncthreads(); // s_sum: thread 0 has read the sums
        if (lane == 0) s_sum[wave][0] = total, s_sum[wave][1] = worst;
        __syncthreads();
        if (tid == 0) {
            total = s_sum[0][0] + s_sum[1][0] + s_sum[2][0] + s_sum[3][0];
            worst = max(max(s_sum[0][1], s_sum[1][1]), max(s_sum[2][1], s_sum[3][1]));
            rec[0] = ok ? 3 : 1, rec[1] = m, rec[2] = s_fit[7], rec[3] = bh;
            for (int k = 0; k < 6; k++) rec[4 + k] = s_fit[k];
            rec[10] = total, rec[11] = worst;
            rec[12] = slot[row + i1], rec[13] = model >= 1 ? slot[row + i2] : -1, rec[14] = model >= 2 ? slot[row + i3] : -1;
            rec[15] = hy.D;
        }
    }
}

} // namespace

LaunchPlan plan_motion_pairs(unsigned long long n_pairs) { return capped_plan(n_pairs, 1, kGridCap); }
LaunchPlan plan_motion_score(unsigned long long n_pairs, int hypotheses)
{
    return capped_plan(n_pairs * (unsigned long long)((hypotheses + kBlock - 1) / kBlock), 1, kGridCap);
}

MotionWs motion_workspace(void *base, int n_pairs, int stride_q, int hypotheses)
{
    // the lists (8 B a slot) | the slots | the counts | m | the pairs
    const size_t slots = (size_t)n_pairs * stride_q;
    MotionWs w;
    w.list = base;
    w.slot = (int *)((Packed *)base + slots);
    w.counts = w.slot + slots;
    w.m = w.counts + (size_t)n_pairs * hypotheses;
    w.pairs = w.m + n_pairs;
    w.bytes = slots * (sizeof(Packed) + sizeof(int)) + (size_t)n_pairs * ((size_t)hypotheses + 3) * sizeof(int);
    return w;
}

hipError_t launch_motion_gather(const long long *q_corners, const int *q_counts, int stride_q, const long long *t_corners,
                                const int *t_counts, int stride_t, int n_pairs, const int *matches, const MotionWs &w,
                                int *inlier, hipStream_t stream)
{
    if (n_pairs < 1 || stride_q < 1 || stride_t < 1 || stride_q > kListMax || stride_t > kHoughMaxLines) return hipErrorInvalidValue;
    const LaunchPlan p = plan_motion_pairs((unsigned long long)n_pairs);
    hipLaunchKernelGGL(motion_gather_kernel, dim3(p.grid), dim3(kBlock), 0, stream, q_corners, q_counts, stride_q, t_corners,
                       t_counts, stride_t, w.pairs, (unsigned)n_pairs, matches, (Packed *)w.list, w.slot, w.m, inlier);
    return hipGetLastError();
}

hipError_t launch_motion_score(int stride_q, int n_pairs, int model, int thr_q4, int hypotheses, unsigned seed,
                               const MotionWs &w, hipStream_t stream)
{
    if (n_pairs < 1 || stride_q < 1 || stride_q > kListMax || model < 0 || model > 2 || thr_q4 < 0 || thr_q4 > 4095 ||
        hypotheses < 1 || hypotheses > kMaxHypotheses)
        return hipErrorInvalidValue;
    const LaunchPlan p = plan_motion_score((unsigned long long)n_pairs, hypotheses);
    const unsigned blocks = (unsigned)((hypotheses + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(motion_score_kernel, dim3(p.grid), dim3(kBlock), 0, stream, (const Packed *)w.list, w.m, stride_q,
                       (unsigned)p.units, blocks, model, thr_q4, hypotheses, seed, w.counts);
    return hipGetLastError();
}

hipError_t launch_motion_refit(int stride_q, int n_pairs, int model, int thr_q4, int hypotheses, unsigned seed,
                               const MotionWs &w, long long *motion, int *inlier, hipStream_t stream)
{
    if (n_pairs < 1 || stride_q < 1 || stride_q > kListMax || model < 0 || model > 2 || thr_q4 < 0 || thr_q4 > 4095 ||
        hypotheses < 1 || hypotheses > kMaxHypotheses)
        return hipErrorInvalidValue;
    const LaunchPlan p = plan_motion_pairs((unsigned long long)n_pairs);
    hipLaunchKernelGGL(motion_refit_kernel, dim3(p.grid), dim3(kBlock), 0, stream, (const Packed *)w.list, w.slot, w.m,
                       stride_q, (unsigned)n_pairs, w.counts, model, thr_q4, hypotheses, seed, motion, inlier);
    return hipGetLastError();
}

} // namespace canny
