// canny_circle_fits.hip -- sub-pixel circle fits: for every Hough circle record the least-squares (Kasa) circle through the
// sub-pixel edgels of the set pixels in a band around the circle, the mean-distance radius, the residuals and the sector
// mask, with one optional trimmed refit, in one 32-byte record.  The rule is part of the interface (include/canny_hip.h,
// DESIGN.md section 25); tests/circle_fits_rule.py restates it in Python ints, canny_circle_fits_host.cpp in plain C++.
//
// One workgroup of four waves per circle slot, grid (centres_max, n_frames), early exit past the frame's count: no grid
// cap, no atomics.
//   walk   : the waves take the rows of the band's bounding box sixteen at a time (wave w: rows 16 w .., then 64 further).
//            Two integer roots per row give the one or two column intervals the band occupies there -- exactly, so every
//            bit of a masked word IS a pixel of the band and no pixel is tested again.  Four lanes share a row, each reads
//            one 64-bit word of its intervals (row_word: words, not pixels), so the words of sixteen rows are in flight
//            together; a shuffle prefix over the popcounts numbers the wave's pixels, and the first kQueueWave of them go
//            into the wave's own part of an LDS queue.  No barrier inside the walk.  (One row per wave and trip, each
//            waiting for its own load, measured 0.58 ms where this measures 0.35, and 0.26 with the third wave per SIMD
//            that the second launch bound keeps: DESIGN.md section 25.)
//   edgels : every queued pixel's edgel record (edgel_record, the edgel kernels' own function) with all lanes busy; the
//            entry becomes (u, v, used).  The three double roots per edgel are paid once per pixel.
//   passes : up to five passes read the queue (moments; distances of the first fit; residuals and, with a trim, the
//            moments of the kept pixels; distances and residuals of the second fit).  Each ends in one reduction -- xor
//            shuffles in the wave, then four partial sums per value through LDS in wave order -- after which every lane
//            holds the sums and the finishing arithmetic is uniform.  Suz and Svz pass 2^63 (see the header): a lane's
//            partial sum fits 64 bits and is split into a high and a low half for the reduction, joined in 128 bits after.
//   rest   : a record with more band pixels than the queue holds walks its rows again in every pass and recomputes the
//            edgels of the pixels past the queue: the same bytes, more slowly.
// Threads 0 and 1 store the record as two 16-byte words.  Plain C++, no inline assembly, no scratch.
#include "canny_line_support.h"
#include "canny_wave.h"

namespace canny {

namespace {

constexpr int kCfBlock = 256;                       // four waves, one circle slot
constexpr int kCfWaves = kCfBlock / 64;
constexpr int kQueueWave = 1024;                    // queued pixels per wave
constexpr int kQueue = kCfWaves * kQueueWave;       // 32 KiB of 8-byte entries: four workgroups per CU by LDS
constexpr int kCfSums = 12;
constexpr int kCfRows = 16;                         // rows of the band per wave and trip

typedef __int128 i128;

// floor(sqrt(v)), exact, 0 <= v < 2^24 (exact as a float; the steps absorb the root's rounding)
__device__ __forceinline__ int cf_isqrt24(int v)
{
    int s = (int)sqrtf((float)v);
    if (s * s > v) s--;
    if ((s + 1) * (s + 1) <= v) s++;
    return s;
}

// floor(sqrt(v)), exact, v < 2^63: the root of the line fits (canny_line_fits.hip), corrected both ways, twice
__device__ __forceinline__ long long cf_isqrt(unsigned long long v)
{
    unsigned long long r = (unsigned long long)sqrt((double)v);
    if (r * r > v) r--;
    if (r * r > v) r--;
    if ((r + 1) * (r + 1) <= v) r++;
    if ((r + 1) * (r + 1) <= v) r++;
    return (long long)r;
}

// a / b to nearest, halves away from zero; b > 0, 2 |a| + b < 2^63
__device__ __forceinline__ long long cf_rdiv(long long a, long long b)
{
    const unsigned long long m = (unsigned long long)(a < 0 ? -a : a);
    const long long q = (long long)((2 * m + (unsigned long long)b) / (2 * (unsigned long long)b));
    return a < 0 ? -q : q;
}

__device__ __forceinline__ int cf_bitlength(i128 v) // v >= 0
{
    const unsigned long long hi = (unsigned long long)(v >> 64), lo = (unsigned long long)v;
    return hi ? 128 - (int)__builtin_clzll(hi) : (lo ? 64 - (int)__builtin_clzll(lo) : 0);
}

struct CfMoments {
    long long n, su, sv, sz, suu, suv, svv;
    i128 suz, svz;
};
struct CfMove {
    long long mx, my; // the centre's move, 1/65536 px
    bool degenerate;
};

// |num| * 2^e / det to nearest, halves away from zero, for a quotient of at most `limit` < 2^19: twenty steps of restoring
// division on 128-bit values.  false: the quotient exceeds the limit.
__device__ __forceinline__ bool cf_quotient(i128 num, int e, long long det, long long limit, long long *out)
{
    const i128 m = num < 0 ? -num : num;
    const i128 X = e > 0 ? m << e : m, Y = e < 0 ? (i128)det << -e : (i128)det;
    if (2 * X >= Y * (2 * limit + 1)) return false;
    i128 R = 2 * X + Y, t = Y << 20; // 2 Y << 19
    long long q = 0;
    for (int i = 19; i >= 0; i--) {
        if (R >= t) R -= t, q |= 1ll << i;
        t >>= 1;
    }
    *out = num < 0 ? -q : q;
    return true;
}

// steps 4 (from the sums on) and 5 of the rule
__device__ __forceinline__ CfMove cf_finish(const CfMoments &m, int band)
{
    CfMove f{0, 0, true};
    if (m.n < 3) return f;
    const i128 A = (i128)m.n * m.suu - (i128)m.su * m.su;
    const i128 B = (i128)m.n * m.suv - (i128)m.su * m.sv;
    const i128 C = (i128)m.n * m.svv - (i128)m.sv * m.sv;
    const i128 P = (i128)m.n * m.suz - (i128)m.su * m.sz;
    const i128 Q = (i128)m.n * m.svz - (i128)m.sv * m.sz;
    i128 top = B < 0 ? -B : B;
    if (A > top) top = A;
    if (C > top) top = C;
    const int bl = cf_bitlength(top), s = bl > 31 ? bl - 31 : 0;
    const long long a = (long long)(A >> s), b = (long long)(B >> s), c = (long long)(C >> s); // arithmetic: floor
    const long long det = a * c - b * b;
    if (det <= 0) return f;
    const long long limit = 65536ll * (band + 2);
    long long mx, my;
    if (!cf_quotient(P * c - Q * b, 7 - s, det, limit, &mx)) return f;
    if (!cf_quotient(Q * a - P * b, 7 - s, det, limit, &my)) return f;
    return CfMove{mx, my, false};
}

// 0..15: quadrants from +x towards +y, four sectors each; a boundary belongs to the sector that starts at it
__device__ __forceinline__ int cf_sector(long long dx, long long dy)
{
    int quad;
    long long p, q;
    if (dx > 0 && dy >= 0)
        quad = 0, p = dx, q = dy;
    else if (dx <= 0 && dy > 0)
        quad = 1, p = dy, q = -dx;
    else if (dx < 0 && dy <= 0)
        quad = 2, p = -dx, q = -dy;
    else if (dx >= 0 && dy < 0)
        quad = 3, p = -dy, q = dx;
    else
        return 0;
    return 4 * quad + (2 * q >= p) + (q >= p) + (q >= 2 * p);
}

struct CfCircle {
    int x2, y2, radius;
    int lo2, hi2;   // (2 lo - 1)^2, (2 (radius + band) + 1)^2
    int ylo, yhi;   // the band's rows inside the frame
};

// Step 2 for the rows of this wave: use(x, y, ordinal) for every pixel of the band in them; the ordinal counts the wave's
// pixels in walk order.  Returns the wave's pixel count (the same in every lane).  A trip takes kCfRows rows at once, four
// lanes to a row, each lane one 64-bit word of the row's intervals (a row with more than four words takes further turns):
// the words of sixteen rows are in flight together, where a row per trip would wait for one load after the other.
template <bool BITS, class Use>
__device__ __forceinline__ int cf_walk(const void *__restrict__ src, const HystGeom &g, int row_bytes, int f,
                                       const CfCircle &c, int wave, int lane, Use &&use)
{
    int count = 0;
    const int sub = lane >> 2, unit = lane & 3;
    for (int y0 = c.ylo + wave * kCfRows; y0 <= c.yhi; y0 += kCfWaves * kCfRows) { // (wave-uniform)
        const int y = y0 + sub;
        int pl = 1, ql = 0, pr = 1, qr = 0; // no interval
        if (y <= c.yhi) {
            const int dy = 2 * y - c.y2, dy2 = dy * dy; // |dy| <= 2 (radius + band): dy2 < hi2
            const int so = cf_isqrt24(c.hi2 - 1 - dy2);  // |2x - x2| <= so
            pl = max((c.x2 - so + 1) >> 1, 0), ql = min((c.x2 + so) >> 1, g.width - 1); // one interval ...
            if (c.lo2 - 1 - dy2 >= 0) { // ... or two, around the pixels with d < lo2
                const int si = cf_isqrt24(c.lo2 - 1 - dy2);
                const int ha = (c.x2 - si + 1) >> 1, hb = (c.x2 + si) >> 1;
                if (ha <= hb) {
                    pr = max(hb + 1, 0), qr = ql;
                    ql = min(ha - 1, g.width - 1);
                }
            }
        }
        const int nl = pl <= ql ? (ql >> 6) - (pl >> 6) + 1 : 0, nr = pr <= qr ? (qr >> 6) - (pr >> 6) + 1 : 0;
        for (int i = unit; __any(i - unit < nl + nr); i += 4) { // (wave-uniform: every lane stays for every turn)
            uint64_t v = 0;
            int k = 0;
            if (i < nl + nr) {
                const bool left = i < nl;
                const int p = left ? pl : pr, q = left ? ql : qr;
                k = (p >> 6) + (left ? i : i - nl);
                const int b0 = max(p - (k << 6), 0), b1 = min(q - (k << 6), 63); // 0 <= b0 <= b1 <= 63
                v = row_word<BITS>(src, g, row_bytes, f, y, k) & ((~0ull >> (63 - b1)) & (~0ull << b0));
            }
            int incl = (int)__popcll(v);
            const int mine = incl;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const int t = __shfl_up(incl, d);
                if (lane >= d) incl += t;
            }
            int ord = count + incl - mine;
            count += __shfl(incl, 63);
            while (v) {
                use((k << 6) + (int)__builtin_ctzll(v), y, ord++);
                v &= v - 1;
            }
        }
    }
    return count;
}

// Step 3 for pixel (x, y): (u, v << 1 | used)
template <class T>
__device__ __forceinline__ uint2 cf_edgel(const T *__restrict__ img, const HystGeom &g, const CfCircle &c, int options,
                                          int x, int y)
{
    const uint4 e = edgel_record(img, g.height, g.width, y, x);
    bool used = true;
    if (options & CANNY_HIP_CIRCLE_FIT_GATE) {
        const long long gx = (int)(short)(e.z & 0xffffu), gy = (int)(short)(e.z >> 16);
        const long long wx = 2 * x - c.x2, wy = 2 * y - c.y2;
        const long long dot = gx * wx + gy * wy;
        used = (gx | gy) && 4 * dot * dot >= 3 * (gx * gx + gy * gy) * (wx * wx + wy * wy);
    }
    if ((options & CANNY_HIP_CIRCLE_FIT_REFINED_ONLY) && !(e.w & CANNY_HIP_EDGEL_REFINED)) used = false;
    const int u = (int)e.x - 128 * c.x2, v = (int)e.y - 128 * c.y2;
    return make_uint2((unsigned)u, ((unsigned)v << 1) | (used ? 1u : 0u));
}

struct CfFit {
    long long mx, my, r;
};
struct CfAcc {
    long long n, su, sv, sz, suu, suv, svv, suz, svz; // suz, svz: this lane's share only
    long long aux;                                    // the sum of e, or Sdd
    int maxd;
    unsigned sectors;
};

__device__ __forceinline__ long long cf_rho(long long u, long long v, const CfFit &f)
{
    const long long U = 256 * u - f.mx, V = 256 * v - f.my;
    return cf_isqrt((unsigned long long)(U * U) + (unsigned long long)(V * V));
}
__device__ __forceinline__ long long cf_resid(long long rho, const CfFit &f) { return (rho - f.r + 128) >> 8; }

// What one used pixel of step 3 adds in pass `pass` (uniform):
//   0: the moments of the first set            1: the distances of the first set against fit 1
//   2: the residuals of the first set against fit 1; with a trim, the moments of the kept pixels
//   3: the distances of the kept pixels against fit 2      4: their residuals against fit 2
__device__ __forceinline__ void cf_add(int pass, long long u, long long v, long long R16, int trim_q8, const CfFit &f1,
                                       const CfFit &f2, CfAcc &a)
{
    bool moments = pass == 0;
    if (pass == 1) a.aux += cf_rho(u, v, f1) - R16;
    if (pass >= 2) {
        long long d = cf_resid(cf_rho(u, v, f1), f1);
        const long long ad1 = d < 0 ? -d : d;
        const bool kept = ad1 <= trim_q8;
        if (pass == 2) moments = trim_q8 > 0 && kept;
        if (pass >= 3 && !kept) return;
        if (pass == 3) a.aux += cf_rho(u, v, f2) - R16;
        if (pass != 3) {
            const CfFit &f = pass == 2 ? f1 : f2;
            if (pass == 4) d = cf_resid(cf_rho(u, v, f2), f2);
            const long long ad = d < 0 ? -d : d;
            a.aux += d * d;
            a.maxd = max(a.maxd, (int)ad);
            a.sectors |= 1u << cf_sector(256 * u - f.mx, 256 * v - f.my);
        }
    }
    if (moments) {
        const long long z = u * u + v * v - (R16 >> 8) * (R16 >> 8); // (256 * radius)^2
        a.n++, a.su += u, a.sv += v, a.sz += z, a.suu += u * u, a.suv += u * v, a.svv += v * v;
        a.suz += u * z, a.svz += v * z;
    }
}

// grid (centres_max, n_frames); one workgroup per circle slot
template <bool BITS, class T>
__global__ __launch_bounds__(kCfBlock, 3) void circle_fits_kernel(const void *__restrict__ src, HystGeom g, int row_bytes,
                                                               const int *__restrict__ circles,
                                                               const int *__restrict__ counts, int centres_max,
                                                               const T *__restrict__ plane, int band, int trim_q8,
                                                               int options, int *__restrict__ fits)
{
    __shared__ uint2 s_queue[kQueue];
    __shared__ long long s_sum[kCfWaves][kCfSums];
    __shared__ int s_max[kCfWaves];
    __shared__ unsigned s_sec[kCfWaves];
    const int f = blockIdx.y, j = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    if (j >= min(centres_max, counts[f])) return; // (workgroup-uniform, as every branch around a barrier below)
    const size_t slot = (size_t)f * centres_max + j;
    const int *rec = circles + slot * 6;
    CfCircle c;
    c.x2 = rec[0], c.y2 = rec[1], c.radius = rec[2];
    int4 *out = reinterpret_cast<int4 *>(fits + slot * CANNY_HIP_CIRCLE_FIT_INTS);
    if (c.radius < 1 || c.radius > kCircleMaxRadius || (unsigned)c.x2 >= 2u * (unsigned)g.width ||
        (unsigned)c.y2 >= 2u * (unsigned)g.height) {
        if (tid < 2) out[tid] = make_int4(tid == 1 ? (int)CANNY_HIP_CIRCLE_FIT_INVALID : 0, 0, 0, 0);
        return;
    }
    const int R = c.radius + band, lo = max(c.radius - band, 1);
    c.lo2 = (2 * lo - 1) * (2 * lo - 1), c.hi2 = (2 * R + 1) * (2 * R + 1); // below 2^23
    c.ylo = max((c.y2 - 2 * R + 1) >> 1, 0), c.yhi = min((c.y2 + 2 * R) >> 1, g.height - 1);
    const T *img = plane + (size_t)f * g.height * g.width;
    uint2 *queue = s_queue + wave * kQueueWave;

    // walk and queue; then the edgels of the queue with every lane busy
    const int count = cf_walk<BITS>(src, g, row_bytes, f, c, wave, lane, [&](int x, int y, int ord) {
        if (ord < kQueueWave) queue[ord].x = (unsigned)(y << 16 | x);
    });
    const int queued = min(count, kQueueWave);
    __syncthreads();
    for (int i = lane; i < queued; i += 64) {
        const unsigned pos = queue[i].x;
        queue[i] = cf_edgel(img, g, c, options, (int)(pos & 0xffffu), (int)(pos >> 16));
    }
    __syncthreads();

    const long long R16 = 65536ll * c.radius;
    CfFit f1{0, 0, 0}, f2{0, 0, 0};
    long long n1 = 0, sdd1 = 0;
    int maxd1 = 0;
    unsigned sec1 = 0;
    for (int pass = 0; pass < 5; pass++) {
        CfAcc a{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0u};
        for (int i = lane; i < queued; i += 64) {
            const uint2 e = queue[i];
            if (e.y & 1u) cf_add(pass, (long long)(int)e.x, (long long)((int)e.y >> 1), R16, trim_q8, f1, f2, a);
        }
        if (count > kQueueWave) // (wave-uniform) the pixels past the queue: walked and computed again
            cf_walk<BITS>(src, g, row_bytes, f, c, wave, lane, [&](int x, int y, int ord) {
                if (ord < kQueueWave) return;
                const uint2 e = cf_edgel(img, g, c, options, x, y);
                if (e.y & 1u) cf_add(pass, (long long)(int)e.x, (long long)((int)e.y >> 1), R16, trim_q8, f1, f2, a);
            });
        // the reduction: in the wave, then the four waves' sums in wave order
        long long v[kCfSums] = {a.n,   a.su,         a.sv,      a.sz,       a.suu,     a.suv,
                                a.svv, a.suz >> 32, a.suz & 0xffffffffll, a.svz >> 32, a.svz & 0xffffffffll, a.aux};
        const bool moments = pass == 0 || (pass == 2 && trim_q8 > 0);
#pragma unroll
        for (int i = 0; i < kCfSums; i++)
            if (i == kCfSums - 1 ? pass != 0 : moments) v[i] = wave_sum(v[i]);
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            a.maxd = max(a.maxd, __shfl_xor(a.maxd, d));
            a.sectors |= (unsigned)__shfl_xor((int)a.sectors, d);
        }
        if (lane == 0) {
#pragma unroll
            for (int i = 0; i < kCfSums; i++) s_sum[wave][i] = v[i];
            s_max[wave] = a.maxd;
            s_sec[wave] = a.sectors;
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < kCfSums; i++) v[i] = s_sum[0][i] + s_sum[1][i] + s_sum[2][i] + s_sum[3][i];
        const int maxd = max(max(s_max[0], s_max[1]), max(s_max[2], s_max[3]));
        const unsigned sectors = s_sec[0] | s_sec[1] | s_sec[2] | s_sec[3];
        __syncthreads(); // every lane has read the sums before the next pass writes them
        const CfMoments m{v[0], v[1], v[2], v[3], v[4], v[5], v[6], ((i128)v[7] << 32) + v[8], ((i128)v[9] << 32) + v[10]};
        if (pass == 0) {
            const CfMove mv = cf_finish(m, band);
            n1 = m.n;
            if (mv.degenerate) {
                if (tid == 0) out[0] = make_int4(32768 * c.x2, 32768 * c.y2, 65536 * c.radius, (int)n1);
                if (tid == 1) out[1] = make_int4((int)CANNY_HIP_CIRCLE_FIT_DEGENERATE, 0, 0, 0);
                return;
            }
            f1.mx = mv.mx, f1.my = mv.my;
        } else if (pass == 1) {
            f1.r = R16 + cf_rdiv(v[11], n1);
        } else if (pass == 2) {
            sdd1 = v[11], maxd1 = maxd, sec1 = sectors;
            const CfMove mv = trim_q8 > 0 ? cf_finish(m, band) : CfMove{0, 0, true};
            if (mv.degenerate) { // no trim, or a trim that failed: the first fit's record
                const unsigned flags = trim_q8 > 0 ? CANNY_HIP_CIRCLE_FIT_TRIM_FAILED : 0u;
                if (tid == 0)
                    out[0] = make_int4((int)(32768ll * c.x2 + f1.mx), (int)(32768ll * c.y2 + f1.my), (int)f1.r, (int)n1);
                if (tid == 1)
                    out[1] = make_int4((int)(((unsigned)maxd1 & CANNY_HIP_CIRCLE_FIT_MAXD_MASK) | flags), (int)sec1,
                                       (int)(unsigned)sdd1, (int)(unsigned)((unsigned long long)sdd1 >> 32));
                return;
            }
            f2.mx = mv.mx, f2.my = mv.my;
            n1 = m.n; // from here on: the kept pixels
        } else if (pass == 3) {
            f2.r = R16 + cf_rdiv(v[11], n1);
        } else {
            if (tid == 0)
                out[0] = make_int4((int)(32768ll * c.x2 + f2.mx), (int)(32768ll * c.y2 + f2.my), (int)f2.r, (int)n1);
            if (tid == 1)
                out[1] = make_int4((int)((unsigned)maxd & CANNY_HIP_CIRCLE_FIT_MAXD_MASK), (int)sectors, (int)(unsigned)v[11],
                                   (int)(unsigned)((unsigned long long)v[11] >> 32));
        }
    }
}

// one lane per moment set: in = 12 long longs (see CANNY_HIP_CIRCLE_FIT_MOMENT_WORDS); out = move_x, move_y, n, flags
__global__ __launch_bounds__(256) void circle_fits_arith_kernel(const long long *__restrict__ in, size_t n,
                                                                int *__restrict__ out)
{
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const long long *p = in + CANNY_HIP_CIRCLE_FIT_MOMENT_WORDS * i;
        const CfMoments m{p[0], p[1], p[2], p[3], p[4], p[5], p[6],
                          (i128)(((unsigned __int128)(unsigned long long)p[8] << 64) | (unsigned long long)p[7]),
                          (i128)(((unsigned __int128)(unsigned long long)p[10] << 64) | (unsigned long long)p[9])};
        const CfMove mv = cf_finish(m, (int)p[11]);
        int *o = out + 4 * i;
        o[0] = (int)mv.mx, o[1] = (int)mv.my, o[2] = (int)m.n;
        o[3] = mv.degenerate ? (int)CANNY_HIP_CIRCLE_FIT_DEGENERATE : 0;
    }
}

} // namespace

int circle_fits_queue_capacity() { return kQueue; }

hipError_t launch_circle_fits(const uint64_t *strong, const uint8_t *bits, const HystGeom &g, const int *circles,
                              const int *counts, int centres_max, const void *plane, bool plane_u8, int band, int trim_q8,
                              int options, int *fits, hipStream_t stream)
{
    const dim3 grid(centres_max, g.n_frames);
    const void *src = bits ? (const void *)bits : (const void *)strong;
    auto launch = [&](auto kernel, auto *img) {
        hipLaunchKernelGGL(kernel, grid, dim3(kCfBlock), 0, stream, src, g, (g.width + 7) / 8, circles, counts, centres_max,
                           img, band, trim_q8, options, fits);
        return hipGetLastError();
    };
    if (bits)
        return plane_u8 ? launch(circle_fits_kernel<true, uint8_t>, (const uint8_t *)plane)
                        : launch(circle_fits_kernel<true, int16_t>, (const int16_t *)plane);
    return plane_u8 ? launch(circle_fits_kernel<false, uint8_t>, (const uint8_t *)plane)
                    : launch(circle_fits_kernel<false, int16_t>, (const int16_t *)plane);
}

hipError_t launch_circle_fits_arith(const long long *moments, size_t n, int *out, hipStream_t stream)
{
    if (!n) return hipSuccess;
    const size_t want = (n + 255) / 256; // no cap: one lane per set
    if (want > 0x7fffffffu) return hipErrorInvalidValue;
    hipLaunchKernelGGL(circle_fits_arith_kernel, dim3((unsigned)want), dim3(256), 0, stream, moments, n, out);
    return hipGetLastError();
}

} // namespace canny
