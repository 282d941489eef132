// canny_shapes.hip -- shape measures of stored contour chains: for every chain of a contours call the polygon moments and
// the point sums relative to the chain's first point, the convex hull of its points, the hull's area and the minimum-area
// rectangle with a side on a hull edge (what cv::moments, cv::convexHull and cv::minAreaRect are asked for right after
// cv::findContours), CSR-shaped over the records.  Everything is integers.  DESIGN.md section 27.
//
// The stage reads what a contours call stored (chain_offsets, points) and runs behind it on the same stream:
//
//   measure : one wave per stored record.  The eleven sums are per-lane partial sums in wrapping 64-bit words, reduced
//             over the wave by one transposing butterfly (17 shuffles for all of them).  The hull starts from the per-column extremes: a point strictly between the smallest and the largest y
//             of its column is no hull vertex, and a closed 8-connected chain covers every column of its bounding box, so
//             the box is at most n columns wide and the candidates arrive sorted by x.  A chain of at most 64 points finds
//             them in registers; a longer one by integer atomicMin / atomicMax into its own point slots of the workspace
//             (minima and maxima: the result does not depend on the order in which they land).  The upper and the lower
//             hull are then rounds of simultaneous elimination: every survivor tests the turn at itself against its
//             surviving neighbours and drops out unless it is strictly convex, until a round removes nothing.  Boxes of at
//             most 64 columns keep the survivors as two 64-bit masks in scalar registers.  Wider ones first run the rounds on
//             every 64 columns by themselves, in registers (what drops out of the hull of a part drops out of the hull of the
//             whole), rank the survivors into a list by ballot and popcount, and go back into registers if at most 64 are
//             left; only beyond that are the rounds re-ranked from one list of the workspace into another.  The finished
//             hull is parked in the workspace, packed (y << 16 | x); hull_offsets[j + 1] receives the count V_h.
//   scan    : hull_offsets[1 .. R] become inclusive prefix sums in place: launch_pg_scan of canny_polygons.hip, unchanged.
//   emit    : one wave per record stores the hull below hull_capacity, sums the shoelace terms, and finds the rectangle with
//             lanes over the edges, an inner loop over the vertices and a wave reduction with the 128-bit comparator, ties
//             going to the smaller edge.
//
// R = min(offsets[n_frames], capacity) is read on the device; the grids are fixed by capacity.  Every output element is
// stored once by one wave, nothing depends on the order in which waves run: the output is the same bytes on every run.
// Every loop is bounded by the chain's length: no input can spin a kernel.  A chain whose bounding box is wider than its
// point count is no 8-connected closed chain; it is answered like a cut one, so no input can write outside its own slots.
#include "canny_kernels.h"
#include "canny_wave.h"

#include <limits.h>

namespace canny {

namespace {

constexpr int kShBlock = 256; // 4 waves: 4 records per workgroup step
constexpr int kShWords = 20;  // CANNY_HIP_SHAPE_WORDS
constexpr int kShSums = 11;   // area2 .. s02

typedef unsigned long long u64;

// The eleven sums of a wave at once, in 17 shuffles of 64 bits instead of 66: at every step of the butterfly a lane keeps half
// of its values and hands the other half to its partner, which keeps those, so 8, 4, 2 and 1 values cross at the distances
// 32, 16, 8 and 4; the one value left is then summed over the distances 2 and 1.  Returns the total of sum number
// (lane >> 2) & 15 (sums 11 .. 15 are zero).
__device__ __forceinline__ u64 sh_wave_sums(const u64 (&s)[11], int lane)
{
    const bool h5 = lane & 32, h4 = lane & 16, h3 = lane & 8, h2 = lane & 4;
    u64 a[8], b[4], c[2];
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const u64 lo = s[k], hi = k + 8 < 11 ? s[k + 8] : 0ull;
        a[k] = (h5 ? hi : lo) + __shfl_xor(h5 ? lo : hi, 32);
    }
#pragma unroll
    for (int k = 0; k < 4; k++) b[k] = (h4 ? a[k + 4] : a[k]) + __shfl_xor(h4 ? a[k] : a[k + 4], 16);
#pragma unroll
    for (int k = 0; k < 2; k++) c[k] = (h3 ? b[k + 2] : b[k]) + __shfl_xor(h3 ? b[k] : b[k + 2], 8);
    u64 d = (h2 ? c[1] : c[0]) + __shfl_xor(h2 ? c[0] : c[1], 4);
    d += __shfl_xor(d, 2);
    d += __shfl_xor(d, 1);
    return d;
}

__device__ __forceinline__ long long sh_cross(long long ax, long long ay, long long bx, long long by)
{
    return ax * by - ay * bx;
}

// The lanes of a wave exchange data through the workspace: stores and atomics of this wave before the fence, loads of this
// wave after it.  The fence is of workgroup scope -- it waits for the wave's own memory operations and moves no cache lines
// (an agent-scope fence adds cache write-backs and invalidates: measured on the 4K batch at min_area 20, this kernel took
// 1.00 ms with it and 0.23 ms without) -- and
// what another lane stored or an atomic changed is read with sh_load, which goes past the L1 to the L2 where both landed.
__device__ __forceinline__ void sh_fence() { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup"); }
__device__ __forceinline__ int sh_load(const int *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the terms of one step (u0, v0) -> (u1, v1) and of the point (u0, v0), added to the eleven sums; wrapping by definition
__device__ __forceinline__ void sh_terms(long long u0, long long v0, long long u1, long long v1, u64 (&s)[kShSums])
{
    const u64 a = (u64)(u0 * v1 - u1 * v0);
    s[0] += a;
    s[1] += a * (u64)(u0 + u1);
    s[2] += a * (u64)(v0 + v1);
    s[3] += a * (u64)(u0 * u0 + u0 * u1 + u1 * u1);
    s[4] += a * (u64)(2 * u0 * v0 + u0 * v1 + u1 * v0 + 2 * u1 * v1);
    s[5] += a * (u64)(v0 * v0 + v0 * v1 + v1 * v1);
    s[6] += (u64)u0;
    s[7] += (u64)v0;
    s[8] += (u64)(u0 * u0);
    s[9] += (u64)(u0 * v0);
    s[10] += (u64)(v0 * v0);
}

// One round of the elimination on a hull half kept as a mask over the lanes (a lane holds one candidate (x, y), x ascending
// with the lane): a survivor between two survivors stays iff sign * turn > 0.  The two ends always stay.  kLaneX: x is the
// lane's own number (consecutive columns), which saves the two shuffles of x.
template <bool kLaneX>
__device__ __forceinline__ u64 sh_round(u64 mask, int lane, int x, int y, int sign)
{
    const u64 below = mask & ((1ull << lane) - 1ull);
    const u64 above = lane == 63 ? 0ull : (mask >> (lane + 1)) << (lane + 1);
    const int pl = below ? 63 - (int)__builtin_clzll(below) : 0;
    const int nl = above ? (int)__builtin_ctzll(above) : 0;
    const int yp = __shfl(y, pl), yn = __shfl(y, nl);
    const int xp = kLaneX ? pl : __shfl(x, pl), xn = kLaneX ? nl : __shfl(x, nl);
    const int xs = kLaneX ? lane : x;
    const long long turn = sh_cross(xs - xp, y - yp, xn - xs, yn - y) * sign;
    const bool alive = (mask >> lane) & 1ull;
    return __ballot(alive && (!below || !above || turn > 0));
}

// sh_round until a round removes nothing: at most 62 rounds remove something
template <bool kLaneX>
__device__ __forceinline__ u64 sh_rounds(u64 mask, int lane, int x, int y, int sign)
{
    for (int guard = 0; guard < 64; guard++) {
        const u64 t = sh_round<kLaneX>(mask, lane, x, y, sign);
        if (t == mask) break;
        mask = t;
    }
    return mask;
}

__device__ __forceinline__ int sh_pack(int x, int y) { return (y << 16) | x; }

#define SH_FOR_EACH_RECORD(n_records, j)                                                                                \
    for (unsigned long long j = ((unsigned long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6,                       \
                            stride_ = ((unsigned long long)gridDim.x * blockDim.x) >> 6;                               \
         j < (n_records); j += stride_)

__device__ __forceinline__ u64 sh_records(const u64 *offsets, int n_frames, u64 capacity)
{
    const u64 total = offsets[n_frames];
    return total < capacity ? total : capacity;
}

// hull_offsets[j + 1] = V_h of record j (0 for a cut chain), hull_offsets[0] = 0; ws: five arrays of point_capacity ints,
// a record's part of each beginning at chain_offsets[j]: col_min | col_max | list A | list B | hull (packed);
// measures[j][0 .. 13] (may be null), (-1, 0, ...) for a cut chain.
__global__ __launch_bounds__(kShBlock) void sh_measure_kernel(const u64 *__restrict__ offsets, int n_frames, u64 capacity,
                                                              const u64 *__restrict__ chain_offsets,
                                                              const int *__restrict__ points, u64 point_capacity, int width,
                                                              u64 *__restrict__ hull_offsets, int *ws,
                                                              long long *__restrict__ measures)
{
    const int lane = threadIdx.x & 63;
    const u64 n_records = sh_records(offsets, n_frames, capacity);
    const u64 lower = (1ull << lane) - 1ull;
    if (blockIdx.x == 0 && threadIdx.x == 0) hull_offsets[0] = 0ull;
    SH_FOR_EACH_RECORD(n_records, j)
    {
        const u64 begin = chain_offsets[j], end = chain_offsets[j + 1];
        long long *m = measures ? measures + kShWords * j : nullptr;
        const bool cut = end > point_capacity || end < begin;
        if (cut || end == begin) {
            if (lane == 0) hull_offsets[j + 1] = 0ull;
            if (m && lane < kShWords) m[lane] = cut && lane == 0 ? -1 : 0;
            continue;
        }
        const u64 n = end - begin;
        const int *p = points + begin;
        int *col_min = ws + begin, *col_max = col_min + point_capacity, *list_a = col_max + point_capacity;
        int *list_b = list_a + point_capacity, *hull = list_b + point_capacity;
        const int p0 = p[0];
        const int y0 = p0 / width, x0 = p0 - y0 * width;
        u64 s[kShSums];
#pragma unroll
        for (int t = 0; t < kShSums; t++) s[t] = 0;
        int left, cols;    // the bounding box's first column and its width
        int ylo = 0, yhi = 0; // boxes of at most 64 columns: the extremes of column left + lane
        if (n <= 64) {
            // ---- one point per lane; the successor over a shuffle; the column extremes in registers ----
            const int nn = (int)n;
            const bool mine = lane < nn;
            const int px = mine ? p[lane] : p0;
            const int y = px / width, x = px - y * width;
            const int nxt = lane + 1 == nn ? 0 : lane + 1;
            const int xn = __shfl(x, nxt), yn = __shfl(y, nxt);
            if (mine) sh_terms(x - x0, y - y0, xn - x0, yn - y0, s);
            left = wave_min(x); // the spare lanes hold P_0
            cols = wave_max(x) - left + 1;
            ylo = INT_MAX, yhi = -1;
            for (int k = 0; k < nn; k++) {
                const int xk = __shfl(x, k), yk = __shfl(y, k);
                if (xk - left == lane) ylo = yk < ylo ? yk : ylo, yhi = yk > yhi ? yk : yhi;
            }
        } else {
            // ---- the lanes stride over the stored points (one step per trip: the eleven sums take the registers) ----
            int xmin = INT_MAX, xmax = -1;
#pragma unroll 1
            for (u64 i = lane; i < n; i += 64) {
                const int pi = p[i], pn = i + 1 < n ? p[i + 1] : p0;
                const int yi = pi / width, xi = pi - yi * width, yn = pn / width, xn = pn - yn * width;
                sh_terms(xi - x0, yi - y0, xn - x0, yn - y0, s);
                xmin = xi < xmin ? xi : xmin, xmax = xi > xmax ? xi : xmax;
            }
            left = wave_min(xmin);
            cols = wave_max(xmax) - left + 1;
        }
        bool bad = (u64)cols > n; // wider than it is long: not an 8-connected closed chain
        if (!bad && n > 64) {
            // ---- the column extremes of a long chain: minima and maxima into the chain's own slots ----
            for (int c = lane; c < cols; c += 64) col_min[c] = INT_MAX, col_max[c] = -1;
            sh_fence();
            for (u64 i = lane; i < n; i += 64) {
                const int pi = p[i];
                const int yi = pi / width, xi = pi - yi * width;
                atomicMin(col_min + (xi - left), yi);
                atomicMax(col_max + (xi - left), yi);
            }
            sh_fence();
            if (cols <= 64 && lane < cols) ylo = sh_load(col_min + lane), yhi = sh_load(col_max + lane);
        }
        if (!bad && cols <= 64) bad = __ballot(lane < cols && yhi < 0) != 0ull; // ... or a column without a point
        if (!bad && cols > 64)
            for (int c0 = 0; c0 < cols; c0 += 64) bad |= __ballot(c0 + lane < cols && sh_load(col_max + c0 + lane) < 0) != 0ull;
        if (bad) { // answered like a cut chain, so that no input can write outside its own slots
            if (lane == 0) hull_offsets[j + 1] = 0ull;
            if (m && lane < kShWords) m[lane] = lane == 0 ? -1 : 0;
            continue;
        }
        unsigned n_hull;
        if (cols <= 64) {
            // ---- the two halves as masks over the columns ----
            const u64 full = cols == 64 ? ~0ull : (1ull << cols) - 1ull;
            u64 top = full, bottom = full;
            for (int guard = 0; guard < 64; guard++) {
                const u64 t = sh_round<true>(top, lane, lane, ylo, 1), b = sh_round<true>(bottom, lane, lane, yhi, -1);
                if (t == top && b == bottom) break;
                top = t, bottom = b;
            }
            const int last = cols - 1;
            const int dup_r = __shfl(ylo, last) == __shfl(yhi, last) ? 1 : 0;
            const int dup_l = cols > 1 && __shfl(ylo, 0) == __shfl(yhi, 0) ? 1 : 0;
            const int n_top = __popcll(top), n_bottom = __popcll(bottom);
            if ((top >> lane) & 1ull) hull[__popcll(top & lower)] = sh_pack(left + lane, ylo);
            const bool skip = (dup_r && lane == last) || (dup_l && lane == 0);
            if (((bottom >> lane) & 1ull) && !skip) {
                const int from_right = __popcll(lane == 63 ? 0ull : bottom >> (lane + 1));
                hull[n_top + from_right - dup_r] = sh_pack(left + lane, yhi);
            }
            n_hull = (unsigned)(n_top + n_bottom - dup_r - dup_l);
        } else {
            // ---- wide boxes.  First every 64 columns on their own, in registers: what drops out of the hull of a part drops
            // out of the hull of the whole.  The survivors of all parts are ranked into a list; if at most 64 are left,
            // they go back into registers, one per lane; otherwise the list is re-ranked round by round in the workspace.
            const int dup_r = sh_load(col_min + cols - 1) == sh_load(col_max + cols - 1) ? 1 : 0;
            const int dup_l = sh_load(col_min) == sh_load(col_max) ? 1 : 0;
            unsigned n_top = 0;
            n_hull = 0;
            for (int half = 0; half < 2; half++) {
                const int *ycol = half ? col_max : col_min;
                const int sign = half ? -1 : 1;
                int *cur = list_a, *nxt = list_b;
                unsigned count = 0;
                for (int c0 = 0; c0 < cols; c0 += 64) {
                    const int c = c0 + lane;
                    const bool valid = c < cols;
                    const int y = valid ? sh_load(ycol + c) : 0;
                    const u64 part = sh_rounds<true>(__ballot(valid), lane, lane, y, sign);
                    if ((part >> lane) & 1ull) cur[count + (unsigned)__popcll(part & lower)] = c;
                    count += (unsigned)__popcll(part);
                }
                sh_fence();
                if (count <= 64) {
                    const int c = lane < (int)count ? sh_load(cur + lane) : 0;
                    const int y = sh_load(ycol + c);
                    const u64 all = count == 64 ? ~0ull : (1ull << count) - 1ull;
                    const u64 mask = sh_rounds<false>(all, lane, c, y, sign);
                    const bool alive = (mask >> lane) & 1ull;
                    const unsigned n_half = (unsigned)__popcll(mask);
                    if (!half) {
                        if (alive) hull[__popcll(mask & lower)] = sh_pack(left + c, y);
                        n_top = n_half;
                    } else {
                        const bool skip = (dup_r && c == cols - 1) || (dup_l && c == 0);
                        const unsigned from_right = (unsigned)__popcll(lane == 63 ? 0ull : mask >> (lane + 1));
                        if (alive && !skip) hull[n_top + from_right - dup_r] = sh_pack(left + c, y);
                        n_hull = n_top + n_half - dup_r - dup_l;
                    }
                    sh_fence(); // the list is free for the other half
                    continue;
                }
                for (int guard = 0; guard < cols; guard++) {
                    unsigned kept = 0;
                    for (unsigned i0 = 0; i0 < count; i0 += 64) {
                        const unsigned i = i0 + lane;
                        const bool valid = i < count, inner = valid && i > 0 && i + 1 < count;
                        const int c = valid ? sh_load(cur + i) : 0, cp = inner ? sh_load(cur + i - 1) : 0, cn = inner ? sh_load(cur + i + 1) : 0;
                        const int y = sh_load(ycol + c), yp = sh_load(ycol + cp), yn = sh_load(ycol + cn);
                        const long long turn = sh_cross(c - cp, y - yp, cn - c, yn - y) * sign;
                        const bool keep = valid && (!inner || turn > 0);
                        const u64 set = __ballot(keep);
                        if (keep) nxt[kept + (unsigned)__popcll(set & lower)] = c;
                        kept += (unsigned)__popcll(set);
                    }
                    sh_fence();
                    int *t = cur;
                    cur = nxt, nxt = t;
                    if (kept == count) break;
                    count = kept;
                }
                if (!half) {
                    for (unsigned i = lane; i < count; i += 64) {
                        const int c = sh_load(cur + i);
                        hull[i] = sh_pack(left + c, sh_load(ycol + c));
                    }
                    n_top = count;
                } else {
                    for (unsigned i = lane; i < count; i += 64) {
                        if ((dup_r && i == count - 1) || (dup_l && i == 0)) continue;
                        const int c = sh_load(cur + i);
                        hull[n_top + (count - 1 - i) - dup_r] = sh_pack(left + c, sh_load(ycol + c));
                    }
                    n_hull = n_top + count - dup_r - dup_l;
                }
                sh_fence(); // the lists are free for the other half
            }
        }
        const u64 total = sh_wave_sums(s, lane); // lanes 0, 4, .. 40 hold the totals of sums 0 .. 10
        if (m && (lane & 3) == 0 && (lane >> 2) < kShSums) m[3 + (lane >> 2)] = (long long)total;
        if (lane == 0) {
            hull_offsets[j + 1] = n_hull;
            if (m) m[0] = (long long)n_hull, m[1] = (long long)n, m[2] = p0;
        }
    }
}

struct ShBest {
    u64 en, len2; // E * N and |d|^2 of the edge
    unsigned k;
    bool have;
};

// a's rectangle is smaller than b's, or as large with the smaller edge
__device__ __forceinline__ bool sh_better(const ShBest &a, const ShBest &b)
{
    if (!a.have || !b.have) return a.have;
    const unsigned __int128 l = (unsigned __int128)a.en * b.len2, r = (unsigned __int128)b.en * a.len2;
    return l < r || (l == r && a.k < b.k);
}

// hull[hull_offsets[j] + k] = the pixel of the k-th hull vertex of record j, below hull_capacity; measures[j][14 .. 19].
// hull_offsets is scanned; ws is as the measure kernel left it.
__global__ __launch_bounds__(kShBlock) void sh_emit_kernel(const u64 *__restrict__ offsets, int n_frames, u64 capacity,
                                                           const u64 *__restrict__ chain_offsets, u64 point_capacity,
                                                           int width, const u64 *__restrict__ hull_offsets,
                                                           const int *__restrict__ ws, int *__restrict__ hull,
                                                           u64 hull_capacity, long long *__restrict__ measures)
{
    const int lane = threadIdx.x & 63;
    const u64 n_records = sh_records(offsets, n_frames, capacity);
    SH_FOR_EACH_RECORD(n_records, j)
    {
        const u64 begin = chain_offsets[j], end = chain_offsets[j + 1];
        if (end > point_capacity || end <= begin) continue; // a cut chain: the measure kernel wrote its measures
        const u64 out_at = hull_offsets[j];
        const unsigned v = (unsigned)(hull_offsets[j + 1] - out_at);
        if (!measures && out_at >= hull_capacity) continue;
        const int *h = ws + 4 * point_capacity + begin;
        if (hull)
            for (unsigned k = lane; k < v; k += 64) {
                const int q = h[k];
                if (out_at + k < hull_capacity) hull[out_at + k] = (q >> 16) * width + (q & 0xFFFF);
            }
        if (!measures || v == 0) continue; // v == 0: the measure kernel refused the chain and wrote its measures
        if (v < 2) {
            if (lane >= 14 && lane < kShWords) measures[kShWords * j + lane] = 0;
            continue;
        }
        long long area = 0;
        ShBest best{0, 0, 0, false};
        long long best_lo = 0, best_hi = 0, best_across = 0;
        for (unsigned k = lane; k < v; k += 64) {
            const int qa = h[k], qb = h[k + 1 == v ? 0 : k + 1];
            const int ax = qa & 0xFFFF, ay = qa >> 16, bx = qb & 0xFFFF, by = qb >> 16;
            area += sh_cross(ax, ay, bx, by);
            const long long dx = bx - ax, dy = by - ay;
            long long lo = 0, hi = 0, across = 0;
            for (unsigned i = 0; i < v; i++) {
                const int q = h[i];
                const long long ex = (q & 0xFFFF) - ax, ey = (q >> 16) - ay;
                const long long al = ex * dx + ey * dy, ac = sh_cross(dx, dy, ex, ey);
                lo = al < lo ? al : lo, hi = al > hi ? al : hi, across = ac > across ? ac : across;
            }
            const ShBest mine{(u64)(hi - lo) * (u64)across, (u64)(dx * dx + dy * dy), k, true};
            if (sh_better(mine, best)) best = mine, best_lo = lo, best_hi = hi, best_across = across;
        }
        ShBest win = best;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            ShBest o;
            o.en = __shfl_xor(win.en, d), o.len2 = __shfl_xor(win.len2, d), o.k = __shfl_xor(win.k, d);
            o.have = __shfl_xor((int)win.have, d) != 0;
            if (sh_better(o, win)) win = o;
        }
        const long long area2 = (long long)wave_sum((u64)area);
        long long *m = measures + kShWords * j;
        if (lane == 0) m[14] = area2;
        if (best.have && best.k == win.k) { // the lane that tried the winning edge
            m[15] = (long long)win.k, m[16] = best_lo, m[17] = best_hi, m[18] = best_across, m[19] = (long long)win.len2;
        }
    }
}

} // namespace

LaunchPlan plan_sh_records(unsigned long long capacity) { return capped_plan(capacity, kShBlock / 64, 1u << 16); }

hipError_t launch_sh_measure(const unsigned long long *offsets, int n_frames, unsigned long long capacity,
                             const unsigned long long *chain_offsets, const int *points, unsigned long long point_capacity,
                             int width, unsigned long long *hull_offsets, int *ws, long long *measures, hipStream_t stream)
{
    hipLaunchKernelGGL(sh_measure_kernel, dim3(plan_sh_records(capacity).grid), dim3(kShBlock), 0, stream, offsets, n_frames,
                       capacity, chain_offsets, points, point_capacity, width, hull_offsets, ws, measures);
    return hipGetLastError();
}

hipError_t launch_sh_emit(const unsigned long long *offsets, int n_frames, unsigned long long capacity,
                          const unsigned long long *chain_offsets, unsigned long long point_capacity, int width,
                          const unsigned long long *hull_offsets, const int *ws, int *hull, unsigned long long hull_capacity,
                          long long *measures, hipStream_t stream)
{
    hipLaunchKernelGGL(sh_emit_kernel, dim3(plan_sh_records(capacity).grid), dim3(kShBlock), 0, stream, offsets, n_frames,
                       capacity, chain_offsets, point_capacity, width, hull_offsets, ws, hull, hull_capacity, measures);
    return hipGetLastError();
}

} // namespace canny
