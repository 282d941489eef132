// canny_binarize.hip -- binarization: gray planes to packed bit maps with a fixed threshold, Otsu's threshold per frame or an
// adaptive (windowed mean) threshold per pixel.  The rule is part of the interface (include/canny_hip.h, DESIGN.md section
// 36); tests/binarize_rule.py restates it in numpy and Python ints, canny_binarize_host.cpp pixel by pixel in plain C++.  All
// integers; every output byte has one writer; the only atomic is the integer sum behind counts[f]: the same bytes on every
// run.
//
//   map      : FIXED and OTSU.  A lane takes eight adjacent pixels and stores one byte; a workgroup takes 256 consecutive
//              output bytes of ONE frame per trip of a capped grid, so the frame's threshold thr[f] and the frame of the count
//              are the same on every lane.  Pad bits are never set.  A lane sums its set bits over its trips; when the frame
//              changes the workgroup reduces them and one lane adds to counts[f].
//   otsu     : one workgroup per frame, a bin per lane: two block prefix sums give w0 and s0, every lane scores its t with a
//              64 x 64 -> 128 product and a restoring division, a wave arg-max (ties to the smaller t) and one lane over the
//              four waves.
//   direct   : ADAPTIVE_MEAN, route 1.  The map's decomposition; a lane sums the kw x kh window of each of its pixels from
//              global memory with clamped coordinates.  Slow and obviously right: the cross-check.
//   marching : ADAPTIVE_MEAN, route 2.  A WAVE takes a strip of 512 useful columns and a segment of rows.  A lane keeps the
//              vertical sums V (kh rows, clamped) of E adjacent staged columns in registers -- 64 E staged columns cover the
//              strip and kw / 2 halo columns a side, the column clamp applied where a row is read -- and a row costs it the
//              entering and the leaving row (the leaving one re-read from the cache: 1 B a pixel, no ring in LDS, so every kh
//              takes the same path).  The horizontal window sum of a row is then a difference of two entries of the prefix
//              sum of V (serial in the lane, wave_inclusive_scan across), which goes through the wave's own LDS row: lane l
//              reads columns l, l + 64, .. (no bank conflict), eight ballots are the row's 64 output bytes, and eight lanes
//              store eight bytes each.  No workgroup barrier: the four waves of a workgroup are independent.  The wave's
//              number is made a scalar (readfirstlane), so its work item and the row loop's branches are scalar too; the
//              next row's loads are issued before the current row is decided, and the loop waits for memory once, at its
//              tail (DESIGN.md section 36 has what the earlier builds waited for).
#include "canny_kernels.h"
#include "canny_wave.h"

namespace canny {

namespace {

constexpr int kBlock = 256;
constexpr unsigned kGridCap = 4096;
constexpr int kStripCols = 512;  // useful columns of a marching strip: 8 a lane
constexpr int kMaxExt = 255;     // CANNY_HIP_BIN_MAX_EXTENT
constexpr int kSmallExt = 65;    // up to here 9 staged columns a lane cover strip + halo (576 = 512 + 64), above 13 (832)

typedef unsigned __int128 u128;

struct BzArgs {
    const void *plane;
    uint8_t *out;
    unsigned long long *counts;
    const int *thr; // map: per frame
    int h, w, rb;
    unsigned long long n_units;
    unsigned trips;
    unsigned chunks;        // bytes kernels: 256-byte chunks of a frame
    unsigned strips, segs;  // marching: of a frame
    int seg_rows;
    int invert, kw, kh, c;
};

template <bool U8>
__device__ __forceinline__ int bz_px(const void *__restrict__ p, size_t i)
{
    return U8 ? (int)static_cast<const uint8_t *>(p)[i] : (int)static_cast<const int16_t *>(p)[i];
}

__device__ __forceinline__ int bz_clamp(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// the division-free form of v > m - c with m = (2 S + A) / (2 A)
__device__ __forceinline__ bool bz_adaptive(int S, int A, int v, int c) { return 2 * S < A * (2 * (v + c) - 1); }

// bytes MSB-first in memory order <- LSB-first word (bit i = column i)
__device__ __forceinline__ uint64_t bz_flip(uint64_t v) { return __builtin_bswap64(__brevll(v)); }

// The workgroup's sum of acc goes to counts[f] by one lane.  Reached by every lane of the workgroup.
__device__ __forceinline__ void bz_flush(unsigned long long *counts, unsigned f, unsigned acc, unsigned *s_part)
{
    const unsigned s = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(counts + f, (unsigned long long)s_part[0] + s_part[1] + s_part[2] + s_part[3]);
    __syncthreads();
}

// FIXED / OTSU (ADAPT = false) and the direct route of ADAPTIVE_MEAN: one output byte a lane.
template <bool U8, bool ADAPT>
__global__ __launch_bounds__(kBlock) void bz_bytes_kernel(BzArgs a)
{
    __shared__ unsigned s_part[4];
    const size_t frame_bytes = (size_t)a.h * a.rb, frame_px = (size_t)a.h * a.w;
    const int ax = a.kw >> 1, ay = a.kh >> 1, A = a.kw * a.kh;
    unsigned acc = 0, cur = 0; // this lane's set bits of frame `cur`, not yet added to counts[cur]
    bool any = false;
    for (unsigned trip = 0; trip < a.trips; trip++) {
        const unsigned long long u = (unsigned long long)blockIdx.x * a.trips + trip;
        if (u >= a.n_units) break; // the same on every lane
        const unsigned f = (unsigned)(u / a.chunks), ch = (unsigned)(u % a.chunks);
        if (a.counts && any && f != cur) { // the same on every lane
            bz_flush(a.counts, cur, acc, s_part);
            acc = 0;
        }
        cur = f, any = true;
        const unsigned b = ch * kBlock + threadIdx.x; // a frame's maps have fewer than 2^28 bytes
        if (b >= frame_bytes) continue;
        const int y = (int)(b / (unsigned)a.rb), x0 = (int)(b - (unsigned)y * (unsigned)a.rb) * 8;
        const size_t base = (size_t)f * frame_px;
        const int t = ADAPT ? 0 : a.thr[f];
        unsigned bits = 0;
        uint64_t eight = 0; // the lane's pixels as bytes where all eight lie in the row: one load at any byte address
        const bool whole = U8 && x0 + 8 <= a.w;
        if (whole) __builtin_memcpy(&eight, static_cast<const uint8_t *>(a.plane) + base + (size_t)y * a.w + x0, 8);
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const int x = x0 + j;
            if (x >= a.w) break; // pad bits are written 0
            const int v = whole ? (int)((eight >> (8 * j)) & 0xffu) : bz_px<U8>(a.plane, base + (size_t)y * a.w + x);
            bool bit;
            if constexpr (ADAPT) {
                int S = 0;
                for (int dy = -ay; dy <= ay; dy++) {
                    const size_t row = base + (size_t)bz_clamp(y + dy, a.h - 1) * a.w;
                    for (int dx = -ax; dx <= ax; dx++) S += bz_px<U8>(a.plane, row + bz_clamp(x + dx, a.w - 1));
                }
                bit = bz_adaptive(S, A, v, a.c);
            } else {
                bit = v > t;
            }
            bits |= (unsigned)(bit != (a.invert != 0)) << (7 - j);
        }
        a.out[(size_t)f * frame_bytes + b] = (uint8_t)bits;
        acc += (unsigned)__popc(bits);
    }
    if (a.counts && any) bz_flush(a.counts, cur, acc, s_part);
}

// floor(ad^2 / den) for den > 0: restoring division, one bit a step (there is no 128-bit division on the device).  The
// remainder stays below den < 2^52, so 64 bits hold it.
__device__ u128 bz_score(unsigned long long ad, unsigned long long den)
{
    u128 n = (u128)ad * ad, q = 0;
    unsigned long long r = 0;
    for (int i = 0; i < 128; i++) {
        r = (r << 1) | (unsigned long long)(n >> 127);
        n <<= 1;
        q <<= 1;
        if (r >= den) r -= den, q |= 1;
    }
    return q;
}

// grid n_frames: thr[f] = the smallest t with the largest score of hist[f] (bin 256 is not read: a u8 plane leaves it empty)
__global__ __launch_bounds__(kBlock) void bz_otsu_kernel(const uint32_t *__restrict__ hist, int *__restrict__ thr)
{
    __shared__ unsigned long long s_scan[4];
    __shared__ unsigned long long s_hi[4], s_lo[4];
    __shared__ int s_t[4];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const unsigned long long hv = hist[(size_t)blockIdx.x * kHistBins + t], hs = hv * (unsigned long long)t;
    unsigned long long N = 0, S = 0;
    const unsigned long long w0 = block_exclusive_scan(hv, s_scan, &N) + hv;
    const unsigned long long s0 = block_exclusive_scan(hs, s_scan, &S) + hs;
    const unsigned long long w1 = N - w0, s1 = S - s0;
    u128 score = 0;
    if (w0 && w1) { // frames of at most 2^26 pixels: both products stay below 2^60
        const long long d = (long long)(w1 * s0) - (long long)(s1 * w0);
        score = bz_score((unsigned long long)(d < 0 ? -d : d), w0 * w1);
    }
    unsigned long long hi = (unsigned long long)(score >> 64), lo = (unsigned long long)score;
    int best = t;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const unsigned long long ohi = __shfl_xor(hi, d), olo = __shfl_xor(lo, d);
        const int ot = __shfl_xor(best, d);
        const bool larger = ohi > hi || (ohi == hi && olo > lo), same = ohi == hi && olo == lo;
        if (larger || (same && ot < best)) hi = ohi, lo = olo, best = ot;
    }
    if (lane == 0) s_hi[wave] = hi, s_lo[wave] = lo, s_t[wave] = best;
    __syncthreads();
    if (t == 0) {
        for (int w = 1; w < 4; w++) // ascending t: only a strictly larger score replaces
            if (s_hi[w] > hi || (s_hi[w] == hi && s_lo[w] > lo)) hi = s_hi[w], lo = s_lo[w], best = s_t[w];
        thr[blockIdx.x] = best;
    }
}

// compiler: the wave's LDS row is written before any lane reads it, and read before it is written again (a wave's LDS
// operations complete in order; no other wave touches the row)
__device__ __forceinline__ void bz_wave_fence() { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); }

// ADAPTIVE_MEAN, marching.  E: staged columns a lane; 64 E >= kStripCols + kw - 1.
template <int E, bool U8>
__global__ __launch_bounds__(kBlock) void bz_march_kernel(BzArgs a)
{
    constexpr int kStage = 64 * E;
    __shared__ unsigned s_p[4][kStage + 1];
    // the wave's number as a scalar: its work item, rows and frame are then scalars too, and the row loop branches on them
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    unsigned *const P = s_p[wave];
    const int ax = a.kw >> 1, ay = a.kh >> 1, A = a.kw * a.kh;
    const size_t frame_px = (size_t)a.h * a.w, frame_bytes = (size_t)a.h * a.rb;
    unsigned acc = 0, cur = 0; // the wave's set bits of frame `cur` (the same on every lane), not yet added to counts[cur]
    bool any = false;
    for (unsigned trip = 0; trip < a.trips; trip++) {
        const unsigned long long u = ((unsigned long long)blockIdx.x * a.trips + trip) * 4 + wave;
        if (u >= a.n_units) break; // the same on every lane of the wave; the kernel has no workgroup barrier
        const unsigned strip = (unsigned)(u % a.strips);
        const unsigned long long r = u / a.strips;
        const unsigned seg = (unsigned)(r % a.segs), f = (unsigned)(r / a.segs);
        if (a.counts && any && f != cur) {
            if (lane == 0) atomicAdd(a.counts + cur, (unsigned long long)acc);
            acc = 0;
        }
        cur = f, any = true;
        const int x0 = (int)strip * kStripCols, y0 = (int)seg * a.seg_rows, y1 = min(a.h, y0 + a.seg_rows);
        // the frame; offsets inside it fit 32 bits (a plane has fewer than 2^31 pixels)
        const uint8_t *const fp = static_cast<const uint8_t *>(a.plane) + (size_t)f * frame_px * (U8 ? 1 : 2);
        const int xs = x0 - ax + lane * E;             // this lane's first staged column
        const bool inside = xs >= 0 && xs + E <= a.w;  // none of them is clamped
        static_assert(E % 4 == 1, "whole words and one byte");
        constexpr int NW = E / 4 + 1;
        // The lane's E staged pixels of row y (clamped) as bytes: column j in bits 8 (j & 3) of word j >> 2.  Loads only, so
        // that the rows a step needs are all in flight before the first is used.
        auto fetch = [&](int y, uint32_t(&wd)[NW]) {
            const unsigned row = (unsigned)bz_clamp(y, a.h - 1) * (unsigned)a.w;
            if (U8 && inside) { // E / 4 words and one byte, at any byte address
                const uint8_t *p = fp + row + xs;
                __builtin_memcpy(wd, p, 4 * (E / 4));
                wd[NW - 1] = p[E - 1];
            } else {
#pragma unroll
                for (int j = 0; j < NW; j++) wd[j] = 0;
#pragma unroll
                for (int j = 0; j < E; j++)
                    wd[j >> 2] |= (uint32_t)bz_px<U8>(fp, row + (unsigned)bz_clamp(xs + j, a.w - 1)) << (8 * (j & 3));
            }
        };
        int V[E];
#pragma unroll
        for (int j = 0; j < E; j++) V[j] = 0;
        auto add = [&](const uint32_t(&wd)[NW], int sign) {
#pragma unroll
            for (int j = 0; j < E; j++) V[j] += sign * (int)((wd[j >> 2] >> (8 * (j & 3))) & 0xffu);
        };
        // the pixels of row y this lane decides: columns x0 + lane + 64 k; beyond the frame the last column, never used
        auto centre = [&](int y, int(&c)[8]) {
            const unsigned row = (unsigned)y * (unsigned)a.w;
#pragma unroll
            for (int k = 0; k < 8; k++) c[k] = bz_px<U8>(fp, row + (unsigned)min(x0 + lane + 64 * k, a.w - 1));
        };
        // The first row's pixels are asked for before the warm-up, whose own waits then cover them: nothing is in flight
        // when the row loop is entered, and its waits count only the loads of the iteration they stand in.
        int cen[8];
        centre(y0, cen);
#pragma unroll 4
        for (int dy = -ay; dy <= ay; dy++) { // the warm-up: kh rows, no output
            uint32_t wd[NW];
            fetch(y0 + dy, wd);
            add(wd, 1);
        }
#pragma unroll 1
        for (int y = y0; y < y1; y++) {
            const bool more = y + 1 < y1; // the same on every lane
            uint32_t enter[NW], leave[NW];
            int next[8];
            if (more) { // the next row's loads fly while this row is decided
                fetch(y + 1 + ay, enter);
                fetch(y - ay, leave);
                centre(y + 1, next);
            }
            unsigned loc = 0;
#pragma unroll
            for (int j = 0; j < E; j++) loc += (unsigned)V[j];
            unsigned run = wave_inclusive_scan(loc, lane) - loc;
            bz_wave_fence(); // the last row's reads come first
#pragma unroll
            for (int j = 0; j < E; j++) {
                P[lane * E + j] = run; // the sum of the staged columns before this one
                run += (unsigned)V[j];
            }
            if (lane == 63) P[kStage] = run;
            bz_wave_fence();
            uint64_t mine = 0;
            unsigned lo[8], hi[8]; // all sixteen reads first: one wait, no branch (col + kw <= kStage on every lane)
#pragma unroll
            for (int k = 0; k < 8; k++) lo[k] = P[lane + 64 * k], hi[k] = P[lane + 64 * k + a.kw];
#pragma unroll
            for (int k = 0; k < 8; k++) {
                const int col = lane + 64 * k;
                const int S = (int)(hi[k] - lo[k]); // staged columns col .. col + kw - 1: x - ax .. x + ax
                // A < 2^17 and |2 (v + c) - 1| < 2^11: the 24-bit product is exact
                const bool cond = 2 * S < __mul24(A, 2 * (cen[k] + a.c) - 1);
                const bool bit = (x0 + col < a.w) & (cond != (a.invert != 0));
                const uint64_t m = __ballot(bit); // bit i: column x0 + 64 k + i; columns >= w stay 0
                acc += (unsigned)__popcll(m);
                if (lane == k) mine = m;
            }
            const int bx = (x0 >> 3) + 8 * lane; // lanes 0..7: the eight bytes of word `lane`
            if (lane < 8 && bx < a.rb) {
                uint8_t *dst = a.out + (size_t)f * frame_bytes + (size_t)y * a.rb + bx;
                const uint64_t raw = bz_flip(mine);
                const int nb = min(8, a.rb - bx);
                if (nb == 8) {
                    __builtin_memcpy(dst, &raw, 8);
                } else {
                    for (int j = 0; j < nb; j++) dst[j] = (uint8_t)(raw >> (8 * j));
                }
            }
            if (more) {
                add(enter, 1);
                add(leave, -1);
#pragma unroll
                for (int k = 0; k < 8; k++) cen[k] = next[k];
            }
        }
    }
    if (a.counts && any && lane == 0) atomicAdd(a.counts + cur, (unsigned long long)acc);
}

bool bz_geom_ok(const void *plane, int n_frames, int h, int w, const uint8_t *out, const unsigned long long *counts)
{
    return plane && out && n_frames >= 1 && n_frames <= 65535 && h >= 1 && w >= 1 && h <= 32768 && w <= 32768 &&
           (long long)h * w < (1ll << 31) && !((uintptr_t)counts & 7);
}

hipError_t bz_zero_counts(unsigned long long *counts, int n_frames, hipStream_t stream)
{
    return counts ? hipMemsetAsync(counts, 0, (size_t)n_frames * sizeof(unsigned long long), stream) : hipSuccess;
}

BzArgs bz_args(const void *plane, int h, int w, uint8_t *out, unsigned long long *counts, int invert)
{
    BzArgs a{};
    a.plane = plane, a.out = out, a.counts = counts, a.h = h, a.w = w, a.rb = (w + 7) / 8, a.invert = invert;
    a.kw = a.kh = 1;
    return a;
}

unsigned bz_chunks(int h, int w) { return (unsigned)(((size_t)h * ((w + 7) / 8) + kBlock - 1) / kBlock); }

} // namespace

LaunchPlan plan_binarize_bytes(int n_frames, int h, int w)
{
    return capped_plan((unsigned long long)bz_chunks(h, w) * (unsigned long long)n_frames, 1, kGridCap);
}

int binarize_strip_cols() { return kStripCols; }

int binarize_staged_cols(int kw) { return 64 * (kw <= kSmallExt ? 9 : 13); }

// A segment pays kh - 1 warm-up rows that only load and add: at least twice as many rows of output bound the overhead, and
// 64 rows keep a wave busy where the window is small.
int binarize_segment_rows(int kh) { return 2 * kh > 64 ? 2 * kh : 64; }

LaunchPlan plan_binarize_march(int n_frames, int h, int w, int kh)
{
    const int seg = binarize_segment_rows(kh);
    const unsigned long long strips = ((unsigned long long)w + kStripCols - 1) / kStripCols, segs = ((unsigned long long)h + seg - 1) / seg;
    return capped_plan(strips * segs * (unsigned long long)n_frames, kBlock / 64, kGridCap);
}

int binarize_auto_route(int kw, int kh)
{
    // the marching route is the faster one at every measured window (3 .. 255, both axes)
    (void)kw, (void)kh;
    return 2;
}

hipError_t launch_binarize_map(const void *plane, bool in_u8, int n_frames, int h, int w, const int *thr, int invert,
                               uint8_t *out, unsigned long long *counts, hipStream_t stream)
{
    if (!bz_geom_ok(plane, n_frames, h, w, out, counts) || !thr || invert < 0 || invert > 1) return hipErrorInvalidValue;
    const hipError_t e = bz_zero_counts(counts, n_frames, stream);
    if (e != hipSuccess) return e;
    const LaunchPlan p = plan_binarize_bytes(n_frames, h, w);
    BzArgs a = bz_args(plane, h, w, out, counts, invert);
    a.thr = thr, a.n_units = p.units, a.trips = (unsigned)p.trips(), a.chunks = bz_chunks(h, w);
    if (in_u8)
        hipLaunchKernelGGL((bz_bytes_kernel<true, false>), dim3(p.grid), dim3(kBlock), 0, stream, a);
    else
        hipLaunchKernelGGL((bz_bytes_kernel<false, false>), dim3(p.grid), dim3(kBlock), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_binarize_otsu(const uint32_t *hist, int n_frames, int *thr, hipStream_t stream)
{
    if (!hist || !thr || n_frames < 1 || n_frames > 65535) return hipErrorInvalidValue;
    hipLaunchKernelGGL(bz_otsu_kernel, dim3(n_frames), dim3(kBlock), 0, stream, hist, thr);
    return hipGetLastError();
}

hipError_t launch_binarize_adaptive(const void *plane, bool in_u8, int n_frames, int h, int w, int c, int kw, int kh,
                                    int invert, int route, uint8_t *out, unsigned long long *counts, hipStream_t stream)
{
    if (!bz_geom_ok(plane, n_frames, h, w, out, counts) || invert < 0 || invert > 1 || c < -255 || c > 255 || kw < 3 ||
        kw > kMaxExt || kh < 3 || kh > kMaxExt || !(kw & 1) || !(kh & 1) || route < 0 || route > 2)
        return hipErrorInvalidValue;
    const hipError_t e = bz_zero_counts(counts, n_frames, stream);
    if (e != hipSuccess) return e;
    BzArgs a = bz_args(plane, h, w, out, counts, invert);
    a.kw = kw, a.kh = kh, a.c = c;
    if ((route ? route : binarize_auto_route(kw, kh)) == 1) {
        const LaunchPlan p = plan_binarize_bytes(n_frames, h, w);
        a.n_units = p.units, a.trips = (unsigned)p.trips(), a.chunks = bz_chunks(h, w);
        if (in_u8)
            hipLaunchKernelGGL((bz_bytes_kernel<true, true>), dim3(p.grid), dim3(kBlock), 0, stream, a);
        else
            hipLaunchKernelGGL((bz_bytes_kernel<false, true>), dim3(p.grid), dim3(kBlock), 0, stream, a);
        return hipGetLastError();
    }
    const LaunchPlan p = plan_binarize_march(n_frames, h, w, kh);
    a.n_units = p.units, a.trips = (unsigned)p.trips(), a.seg_rows = binarize_segment_rows(kh);
    a.strips = (unsigned)((w + kStripCols - 1) / kStripCols), a.segs = (unsigned)((h + a.seg_rows - 1) / a.seg_rows);
    const dim3 grid(p.grid), block(kBlock);
    if (kw <= kSmallExt) {
        if (in_u8)
            hipLaunchKernelGGL((bz_march_kernel<9, true>), grid, block, 0, stream, a);
        else
            hipLaunchKernelGGL((bz_march_kernel<9, false>), grid, block, 0, stream, a);
    } else {
        if (in_u8)
            hipLaunchKernelGGL((bz_march_kernel<13, true>), grid, block, 0, stream, a);
        else
            hipLaunchKernelGGL((bz_march_kernel<13, false>), grid, block, 0, stream, a);
    }
    return hipGetLastError();
}

} // namespace canny
